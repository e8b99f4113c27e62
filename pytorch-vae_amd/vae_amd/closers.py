"""The losses that close a forward in place of the ELBO and write the backward's dL/drecon seed
themselves: the Autoencoder's centre-weighted MSE and MS-SSIM (models/autoencoder.py:230-267,
vae_recon_loss) and LogCoshVAE's log-cosh term with its KL (models/logcosh_vae.py:125-155,
vae_logcosh_loss).  A fused training StepPlan built with recon_loss= or with a loss in CLOSERS holds
one as `plan.closer`; the drop-in models evaluate the same object on their own tensors (evaluate,
from models._HipReconLoss / _HipLogCosh).

A closer owns its argument struct `args` (the loss's constants, from _lib.recon_loss_args /
logcosh_args), the workspace the kernel asks for, and whatever else the struct points at for as long
as it may be launched (the fp32 mask, the tensors of `point`).  It also says which calls its kernel
takes (takes) — the models fall back to torch for the others."""
from __future__ import annotations

import torch

from . import _lib as L


class Closer:
    fn = None               # the kernel
    result = 0              # the entry of `out` that is the drop-in's reconstruction loss
    ws_dtype = None         # the workspace's element type
    ws_query = None         # _lib's workspace query of `args`

    def __init__(self, args, device, keep=None):
        self.args, self.keep = args, keep           # (keep: what else `args` points at — the fp32 mask)
        size = torch.finfo(self.ws_dtype).bits // 8
        self.ws = torch.zeros(max(1, self.ws_query(args) // size), dtype=self.ws_dtype, device=device)
        args.workspace, args.workspace_bytes = self.ws.data_ptr(), self.ws.numel() * size

    def point(self, *, recon, target, grad, out, **more):
        """The tensors of a call: the reconstruction, its target, dL/drecon and the loss terms ([4]);
        in a step also the head's `sse` and `per_img`."""
        self.at = dict(recon=recon, target=target, grad=grad, out=out, **more)
        for field, t in self.at.items():
            setattr(self.args, field, t.data_ptr())
        return self

    def join(self, plan, F, **more):
        """The call closing a plan's forward: loss terms into `out`, per-image MSE from the head's SSE,
        dL/drecon into grad_recon for the backward."""
        self.point(recon=plan.recon, target=plan.x, grad=plan.grad_recon, out=plan.out, sse=plan.sse,
                   per_img=plan.per_img, **more)
        plan._add(F, self.fn, self.args)

    def run(self, stream):
        L.call(self.fn, self.args, stream)

    @classmethod
    def evaluate(cls, recons: torch.Tensor, target: torch.Tensor, *cfg):
        """The drop-in path: the loss of these tensors, at once on the current stream.  Returns the
        reconstruction loss and dL/drecons."""
        recons, target = recons.detach().float().contiguous(), target.detach().float().contiguous()
        grad = torch.empty_like(recons)
        out = torch.zeros(4, dtype=torch.float32, device=recons.device)
        closer = cls(recons.shape, recons.device, *cfg).point(recon=recons, target=target, grad=grad, out=out)
        closer.run(L.stream_ptr())
        return out[cls.result].clone(), grad


class ReconLoss(Closer):
    """vae_recon_loss over [n][c][h][w] images.  `cfg` is StepPlan's recon_loss dict: {"kind": "center",
    "mask": [h][w] tensor} or {"kind": "mssim", "window": 1-D window[, "levels": 5, "normalize": True]}."""
    fn, ws_dtype, ws_query = "vae_recon_loss", torch.float32, staticmethod(L.recon_loss_workspace)

    def __init__(self, shape, device, cfg: dict):
        n, c, h, w = shape
        if cfg["kind"] == "center":
            kind, kw = L.RLOSS_CENTER, dict(mask=cfg["mask"].to(device, torch.float32).contiguous().view(h, w))
        elif cfg["kind"] == "mssim":
            kind, kw = L.RLOSS_MSSIM, dict(window=cfg["window"], levels=cfg.get("levels", 5),
                                           normalize=cfg.get("normalize", True))
        else:
            raise ValueError(f"recon_loss kind {cfg['kind']!r}")
        super().__init__(L.recon_loss_args(kind, n, c, h, w, **kw), device, kw)

    @classmethod
    def for_plan(cls, plan, *, recon_loss, **_):
        return cls(plan.recon.shape, plan.net.device, recon_loss)

    @staticmethod
    def takes_planes(recons, target) -> bool:
        """The part of `takes` that needs no cfg (a model builds its cfg only for such tensors)."""
        return (recons.is_cuda and recons.dim() == 4 and recons.shape[2] * recons.shape[3] <= 4096
                and recons.shape[2:] == target.shape[2:])

    @staticmethod
    def takes(cfg, recons, target) -> bool:
        """Whether the kernel takes this call: CUDA images of equal planes of at most 4096 pixels; an
        MS-SSIM pyramid that halves exactly (other plane sizes: the reference's avg_pool2d floors
        them, mssim_vae.py); a centre mask of the plane's shape."""
        if cfg is None or not ReconLoss.takes_planes(recons, target):
            return False
        if cfg["kind"] == "mssim":
            step = 1 << (cfg.get("levels", 5) - 1)
            return not (recons.shape[2] % step or recons.shape[3] % step)
        return cfg["kind"] != "center" or tuple(cfg["mask"].shape) == tuple(recons.shape[2:])


class LogCoshLoss(Closer):
    """vae_logcosh_loss over [n][c][h][w] images: the log-cosh term alone (the drop-in: no mulv), or in a
    step with the KL of mu | log_var weighted kl_weight = beta * M_N and its coefficient into kl_coef."""
    fn, result, ws_dtype, ws_query = "vae_logcosh_loss", 1, torch.float64, staticmethod(L.logcosh_workspace)

    def __init__(self, shape, device, alpha: float, kl_weight: float = 0.0, latent: int = 0):
        n, c, h, w = shape
        super().__init__(L.logcosh_args(n, c * h * w, alpha, latent=latent, kl_weight=kl_weight), device)

    @staticmethod
    def check(*, alpha, samples, recon_loss):
        """A plan's arguments, before anything is built.  (alpha's default in StepPlan is InfoVAE's: the
        log-cosh plan has to be given its own.)"""
        if recon_loss is not None or samples != 1:
            raise ValueError("StepPlan(loss='logcosh') takes one sample and no recon_loss")
        if not 0.0 < float(alpha) < float("inf"):
            raise ValueError(f"StepPlan(loss='logcosh') needs a finite alpha > 0, got {alpha}")

    @classmethod
    def for_plan(cls, plan, *, alpha, beta, **_):
        return cls(plan.recon.shape, plan.net.device, float(alpha), kl_weight=float(beta) * plan.kld_weight,
                   latent=plan.net.latent_dim)

    def join(self, plan, F):
        """... and the KL coefficient beta*kld_weight/B into kl_coef."""
        super().join(plan, F, mulv=plan.mulv, kl_coef=plan.kl_coef)

    @staticmethod
    def takes(alpha, recons, target) -> bool:
        return recons.is_cuda and recons.dim() == 4 and recons.shape == target.shape and float(alpha) > 0.0


# loss name -> the closer a fused training plan of that loss ends its forward with; such a loss never
# runs on the ELBO kernel.  (recon_loss= is an argument of its own: it selects ReconLoss.)
CLOSERS = {"logcosh": LogCoshLoss}
