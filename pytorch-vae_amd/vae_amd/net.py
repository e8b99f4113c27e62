"""The VanillaVAE-family network on libvaehip (VanillaVAE, BetaVAE, IWAE share it).

Reference: models/vanilla_vae.py:11-146 (network, reparameterize, ELBO), beta_vae.py:129-152,
iwae.py:95-160, experiment.py:45-86 (the step that calls it), experiment.py:308-311 (Adam).

Design (MI355X-first):
  * weights live in one flat fp32 buffer in native layouts (layout.py); in bf16 mode a bf16
    copy of the GEMM weights is refreshed by the fused Adam kernel;
  * activations are NHWC and stored *pre-BatchNorm*: every BatchNorm+LeakyReLU is applied by
    the consuming kernel on load, the producing kernel accumulates Σ/Σ² per channel in its
    epilogue, and backward folds BN-backward into the next kernel's load the same way;
  * a `StepPlan` preallocates every buffer for one batch shape and prebuilds the ctypes
    argument blocks of the ~40 launches of a training step, so a step is a fixed launch
    sequence on one stream — capturable into a HIP graph (engine.py).
"""
from __future__ import annotations

import ctypes
from typing import Dict, List, Optional

import torch

from . import _lib as L
from .calls import BATCH_FN, batch_filter_calls, call_one, run_calls, size_workspaces, structs  # noqa: F401
from .layout import reference_key_order, vanilla_layout
from .plan import NetBase, PlanBase, ZeroRegion, _pad4, make_swaps                              # noqa: F401
from .closers import CLOSERS, ReconLoss
from .terms import MMD_KINDS, TERMS

SLOPE = 0.01         # nn.LeakyReLU default
# layers at least this large take materialised operands by default (StepPlan.big_layer,
# StepPlan(mat_min_flops=...))
MAT_MIN_FLOPS = 4e9
BN_EPS = 1e-5
BN_MOMENTUM = 0.1


class VAENet(NetBase):
    """Parameters + BatchNorm state of the VanillaVAE conv stack on one device."""

    swaps_in_step_begin = True      # (make_swaps: one array of <= SWAP_MAX weights)

    def __init__(self, in_channels: int = 3, latent_dim: int = 128, hidden_dims: Optional[List[int]] = None,
                 img_size: int = 64, dtype: torch.dtype = torch.float32, device=None,
                 generator: Optional[torch.Generator] = None):
        self.in_channels = in_channels
        self.latent_dim = latent_dim
        self.hidden_dims = list(hidden_dims or [32, 64, 128, 256, 512])
        self.img_size = img_size
        if img_size % (2 ** len(self.hidden_dims)) or img_size // (2 ** len(self.hidden_dims)) != 2:
            raise ValueError("the reference's bottleneck is a [C,2,2] map (fc_mu = hidden_dims[-1]*4, "
                             "models/vanilla_vae.py:36): need img_size == 2 * 2**len(hidden_dims)")
        if in_channels != 3:
            raise ValueError("the head reconstructs 3 channels (vanilla_vae.py:73); in_channels must be 3")
        super().__init__(vanilla_layout(in_channels, latent_dim, self.hidden_dims),
                         reference_key_order(in_channels, latent_dim, self.hidden_dims), dtype, device, generator)
        if self.lowp is not None:
            # bf16 mode: swapped-axes copies (vaehip.h wt_t) of the weights the bf16 GEMMs read
            # transposed — every ConvTranspose2d (its forward) and every Conv2d with a data gradient
            # (encoder blocks 1..) — refreshed with the bf16 copy (sync_lowp / FusedAdam.apply)
            names = ([f"encoder.{i}.0.weight" for i in range(1, len(self.hidden_dims))] +
                     [f"decoder.{i}.0.weight" for i in range(len(self.hidden_dims) - 1)] + ["final_layer.0.weight"])
            descs, self.lowp_t = make_swaps(self.layout, self.params, names, self.device, self.wt_t, self.lowp)
            self.swap_descs = [descs]
        self.sync_lowp()

    def run_stats(self, prefix: str):
        """Pointers of a BatchNorm's running mean and running variance."""
        b = self.layout.bn_by_prefix[prefix]
        return self.running.data_ptr() + 4 * b.offset, self.running.data_ptr() + 4 * (b.offset + b.channels)


class StepPlan(PlanBase):
    """All buffers and prebuilt launches of one training step for a fixed batch shape.

    loss: 'vanilla' | 'betaH' | 'betaB' | 'iwae' | 'info' | 'dip' | 'miwae' | 'logcosh';  samples: IWAE S
    (decoder batch B*S).
    'miwae' (MIWAE, models/miwae.py:124-164) takes samples = K and estimates = M: S = M*K rows per image
    in b, m, k order, IWAE's weighting inside each group of K (VAE_LOSS_MIWAE).
    'info' (InfoVAE, models/info_vae.py:128-229) takes alpha, beta, reg_weight, kernel_type and
    latent_var; its MMD term runs on vae_mmd_fwd right after the reparameterization.
    'dip' (DIP-VAE, models/dip_vae.py:125-164) takes lambda_diag and lambda_offdiag; its covariance
    penalty runs on vae_dip_fwd as soon as mu | log_var are final.
    'logcosh' (LogCoshVAE, models/logcosh_vae.py:125-155) takes alpha (> 0, to be given: the default is
    InfoVAE's) and beta; vae_logcosh_loss closes its forward in place of the ELBO and seeds the backward
    with dL/drecon (grad_recon) and the KL coefficient beta*kld_weight/B (kl_coef).
    Such a batch-coupled latent term is `self.term` (terms.py) of a training plan, None otherwise.
    A loss that closes the forward in place of the ELBO — recon_loss=, or a loss in CLOSERS — is
    `self.closer` (closers.py) of a fused training plan, None otherwise.
    grads land in `self.grads` (same layout as net.params); `zero` (grads, BN sums, SSE,
    d[mu|logvar]) is cleared by `vae_step_begin` at the start of every step."""

    def __init__(self, net: VAENet, batch: int, *, loss: str = "vanilla", kld_weight: float = 1e-8,
                 samples: int = 1, beta: float = 4.0, gamma: float = 1000.0, max_capacity: float = 25.0,
                 capacity_max_iter: float = 1e5, fused_loss: bool = True, training: bool = True,
                 concurrent: bool = False, fuse_bn: bool = False, bn_in_consumer: bool = True,
                 wg_overlap: bool = False, recon_loss: Optional[dict] = None,
                 deterministic: Optional[bool] = None, latent_kernels: bool = True, head_kernels: bool = True,
                 pad_rgb: bool = True, materialise: bool = True, mat_min_flops: float = MAT_MIN_FLOPS,
                 batch_wgrads: bool = True, alpha: float = -0.5, reg_weight: float = 100.0,
                 kernel_type: str = "imq", latent_var: float = 2.0, lambda_diag: float = 10.0,
                 lambda_offdiag: float = 5.0, estimates: Optional[int] = None):
        # Route options (explicit arguments; every non-default route has a GPU test,
        # tests/test_gpu_routes.py): latent_kernels / head_kernels / pad_rgb / materialise /
        # batch_wgrads = False keep the generic per-op calls in place of the dedicated bottleneck
        # kernels, the 64/128-channel head kernels, the 8-channel padded RGB ends, materialised
        # BatchNorm operands for layers >= mat_min_flops, and the batched weight gradients.
        if loss in CLOSERS:
            CLOSERS[loss].check(alpha=alpha, samples=samples, recon_loss=recon_loss)
        super().__init__(net)
        self.materialise, self.mat_min_flops = bool(materialise), float(mat_min_flops)
        self.batch_wgrads_on = bool(batch_wgrads)
        # deterministic: every cross-workgroup reduction of the step in a fixed order (vaehip.h
        # vae_conv_args.deterministic), so two runs of the same step give bit-identical gradients;
        # the default for fp32 (parity) plans, unsupported by the bf16 kernels.
        self.deterministic = (net.dtype == torch.float32) if deterministic is None else bool(deterministic)
        # closing: the class of the loss that closes the forward in place of the ELBO and seeds the
        # backward with its dL/drecon (grad_recon), as the drop-in path does with autograd's —
        # recon_loss= (the Autoencoder's other reconstruction losses: {"kind": "center", "mask": [H][W]
        # tensor} or {"kind": "mssim", "window": 1-D window}) or a loss in CLOSERS.  Fused training plans
        # only: the drop-in's loss is the caller's, an eval plan has no loss call.
        closing = (ReconLoss if recon_loss is not None else CLOSERS.get(loss)) if training and fused_loss else None
        self.seed_recon = (not fused_loss) or closing is not None
        self.B = batch
        # training=False: eval-mode BatchNorm (running statistics, nothing updated; the
        # reference's validation_step / sample / generate under model.eval()) — forward only
        self.training = training
        # fused_loss: the ELBO runs on the GPU inside the step and seeds the backward itself.
        # False (the BaseVAE drop-in, vae_amd.models): the loss is computed by the caller from
        # recon/mu/log_var and the backward is seeded with dL/drecon (grad_recon) and
        # dL/d[mu|log_var] (written into dmulv) instead.
        self.fused_loss = fused_loss
        # bn_in_consumer: no vae_bn_finalize launches in training — every kernel that applies a
        # BatchNorm reduces the producer's replicated statistics itself (vae_common.hpp
        # tab_build); the forward consumer's first workgroup updates the running statistics and
        # the weight-gradient call's first workgroup writes dL/dgamma, dL/dbeta and the conv
        # bias gradient (closed form).  Eval mode keeps vae_bn_finalize (running statistics).
        self.bn_in_consumer = bn_in_consumer and training
        # estimates (MIWAE's M): S = M*K rows per image; every other loss has one group of `samples`
        if estimates is not None and loss != "miwae":
            raise ValueError(f"estimates is MIWAE's argument, not loss {loss!r}'s")
        self.M = 1
        if loss == "miwae":
            self.M = 1 if estimates is None else int(estimates)
            if self.M < 1 or int(samples) < 1:
                raise ValueError(f"StepPlan(loss='miwae') needs samples >= 1 and estimates >= 1, "
                                 f"got {samples} and {estimates}")
            if not 1 <= batch <= 1024:
                raise ValueError(f"StepPlan(loss='miwae') takes 1..1024 images a batch (vae_elbo_fwd), got {batch}")
        self.S = samples if loss == "iwae" else (self.M * int(samples) if loss == "miwae" else 1)
        self.loss, self.loss_kind = loss, self.LOSS_KINDS[loss]
        self.kld_weight, self.beta, self.gamma = kld_weight, beta, gamma
        if kernel_type not in MMD_KINDS:
            raise ValueError('Undefined kernel type.')                   # info_vae.py:173
        if loss in TERMS and fused_loss and not training:
            # an eval plan has no MMD / DIP call (nothing to seed), so the fused ELBO would find no
            # partials: the loss of an eval forward is the caller's (models.InfoVAE, models.DIPVAE)
            raise ValueError(f"StepPlan(loss='{loss}', training=False) has no fused loss: pass fused_loss=False")
        self.max_capacity, self.capacity_max_iter = max_capacity, capacity_max_iter
        dev, T = net.device, net.dtype
        D, h, img = net.latent_dim, net.hidden_dims, net.img_size
        B, BS = self.B, self.B * self.S
        # latent: the bottleneck (fc_mu|fc_var, reparameterize, decoder_input and their backward) on
        # the vae_latent_* kernels — two launches each way instead of nine (vaehip.h).  bf16 training
        # plans with the fused loss (the TrainStep engine) and the shapes those kernels take;
        # latent_kernels=False keeps the per-op calls.
        C5, r0 = net.hidden_dims[-1], net.hidden_dims[::-1][0]
        self.latent_fused = (T == torch.bfloat16 and training and fused_loss and net.latent_dim in (64, 128)
                             and C5 % 128 == 0 and (4 * r0) % 128 == 0 and net.img_size == 64
                             and latent_kernels)
        # wide_head: a final layer wider than the head kernels take on MFMA (bf16, 64-wide images:
        # 32, 64 or 128 channels — configs/big_ae.yaml's 128 included) runs the head Conv2d(C->3)
        # on the conv-GEMM paths with its 3 outputs zero-padded to 8, then vae_recon_fwd (tanh, NCHW
        # reconstruction, SSE, backward seed) — the VQ-VAE output layer's route (the Autoencoder's
        # 256-512-channel final layers, and the fp32 parity mode above 32).  The reconstruction seed
        # is the mean-MSE one, so not for IWAE's per-sample weights (S > 1 keeps the head kernels).
        # head_kernels=False keeps the conv-GEMM route for 64/128 channels.
        head_mfma = T == torch.bfloat16 and img == 64 and h[0] in (64, 128) and head_kernels
        self.wide_head = h[0] > 32 and self.S == 1 and not head_mfma

        # -------- buffers
        f32 = dict(dtype=torch.float32, device=dev)
        self.x = torch.zeros(B, 3, img, img, **f32)                     # NCHW input (reference layout)
        # bf16: the image and the first conv's weights carried as 8 zero-padded channels (packed
        # GEMM operands; vae_nchw_to_nhwc_pad / vae_pad_channels at the start of every step)
        self.pad_rgb = T == torch.bfloat16 and pad_rgb
        if self.pad_rgb:
            self.x8 = torch.zeros(B, img, img, 8, dtype=T, device=dev)
            self.w8 = torch.zeros(h[0] * 9 * 8, dtype=T, device=dev)
        self.eps = torch.zeros(BS, D, **f32)
        self.enc = [torch.empty(B, img >> (i + 1), img >> (i + 1), c, dtype=T, device=dev) for i, c in enumerate(h)]
        self.mulv = torch.empty(B, 2 * D, **f32)
        self.z = torch.empty(BS, D, dtype=T, device=dev)
        r = h[::-1]
        self.h0 = torch.empty(BS, 2, 2, r[0], dtype=T, device=dev)
        self.dec = [torch.empty(BS, 4 << i, 4 << i, c, dtype=T, device=dev) for i, c in enumerate(r[1:])]
        self.fin = torch.empty(BS, img, img, r[-1], dtype=T, device=dev)
        if self.wide_head:
            # the head's output (pre-tanh) and its gradient, 8 channels (3 real); the head weights
            # zero-padded to 8 output rows (vae_pad_channels at the step's head: rows 3..7 stay 0)
            self.y8 = torch.zeros(BS, img, img, 8, dtype=T, device=dev)
            self.g8 = torch.zeros(BS, img, img, 8, dtype=T, device=dev)
            self.w8h = torch.zeros(8 * 9 * r[-1], dtype=T, device=dev)
            self.b8h = torch.zeros(8, dtype=torch.float32, device=dev)   # bias padded alike (lanes 3..7 stay 0)
        self.recon = torch.empty(BS, 3, img, img, **f32)
        self.grad_recon = torch.zeros(BS, 3, img, img, **f32) if self.seed_recon else None
        self.out = torch.zeros(4, **f32)                                  # loss, recon, KLD(report), kld
        self.per_img, self.head_coef, self.kl_coef = (torch.zeros(BS, **f32) for _ in range(3))
        self.num_iter = torch.zeros(1, **f32)                             # BetaVAE-B counter (beta_vae.py:132)
        # backward buffers (gradients w.r.t. pre-activation of each stored tensor)
        self.g_enc = [torch.empty_like(t) for t in self.enc]
        self.g_h0 = torch.empty_like(self.h0)
        self.g_dec = [torch.empty_like(t) for t in self.dec]
        self.g_fin = torch.empty_like(self.fin)
        # zero region: grads | BN statistics | sse | dmulv   (16-B aligned pieces).  Every
        # BatchNorm has forward sums (Σ, Σ²) and backward sums (Σg·x̂, Σg), each kept in
        # `bn_reps(C)` replicas so that the producing kernels' per-block atomics spread out.
        bn_shape = {b.prefix: (2, bn_reps(b.channels), b.channels) for b in net.layout.bns}
        zr = ZeroRegion()
        zr.add("grads", net.layout.total)
        # loss terms averaged over ranks (experiment.py:55 log_dict(sync_dist=True)): copied from
        # `out` after the forward and reduced together with the last gradient bucket (engine.py)
        zr.add("metrics", 4)
        for p, (_, reps, c) in bn_shape.items():
            zr.add("bnfwd." + p, 2 * reps * c, pad=False)       # [2][reps][C]: Σ(y-shift), Σ(y-shift)²
            zr.add("bnbwd." + p, 2 * reps * c, pad=False)       # [2][reps][C]: Σg·x̂ (dγ), Σg (dβ)
        zr.add("sse", BS)
        zr.add("dmulv", B * 2 * D)
        zr.add("counters", 2 * len(bn_shape))
        if self.latent_fused:       # vae_latent_fc_fwd accumulates mu|log_var: zero at every step
            zr.add("mulv", B * 2 * D)
        if self.wide_head:          # the padded head's weight / bias gradients (vae_unpad_accumulate)
            zr.add("dw8h", 8 * 9 * r[-1])
            zr.add("db8h", 8)
        z = zr.alloc(dev)
        self.zero, self.grads, self.metrics, self.sse, self.dmulv = (z[k] for k in ("zero", "grads", "metrics", "sse", "dmulv"))
        self.bnfwd = {p: z["bnfwd." + p].view(s) for p, s in bn_shape.items()}
        self.bnbwd = {p: z["bnbwd." + p].view(s) for p, s in bn_shape.items()}
        self.counters = z["counters"].view(torch.int32)
        if self.latent_fused:
            self.mulv = z["mulv"].view(B, 2 * D)
        self.dw8h, self.db8h = z.get("dw8h"), z.get("db8h")
        # per-BatchNorm coefficient tables, rewritten every step by vae_bn_finalize:
        # forward [4][C] (BN_ACT) then backward [3][C] (BN_DY)
        self.bntab: Dict[str, torch.Tensor] = {
            b.prefix: torch.zeros(7 * b.channels, **f32) for b in net.layout.bns}
        self.step = torch.zeros(1, dtype=torch.int32, device=dev)
        # side stream for the weight gradients (run_calls); None: one stream
        self.side = torch.cuda.Stream(device=dev) if (concurrent and training) else None
        # wg_overlap: the decoder's weight gradients (one batch) on a side stream, beside the
        # encoder's data-gradient chain (batch_wgrads); one fork and one join per step.  Off by
        # default: measured 0.670 vs 0.648 ms/step (B=64, graph-replayed) — the graph's cross-stream
        # edges cost more than the overlap gains, as the per-call side stream of round 1 did
        self.wg_overlap = wg_overlap and training and not concurrent
        self._mat_a: Dict[str, torch.Tensor] = {}         # materialised lrelu(BN(y)) per BatchNorm
        self._mat_dz: Dict[str, torch.Tensor] = {}        # materialised BN-backward gradients
        self.side_all = self.side is not None            # concurrent: every weight-gradient call
        if self.wg_overlap:
            self.side = torch.cuda.Stream(device=dev)
        # the loss's batch-coupled latent term (InfoVAE's MMD, DIP-VAE's covariance penalty), with
        # its buffers and its call; an eval plan has none (nothing to seed)
        self.term = None
        if loss in TERMS and training:
            self.term = TERMS[loss](self, alpha=alpha, reg_weight=reg_weight, kernel_type=kernel_type,
                                    latent_var=latent_var, lambda_diag=lambda_diag, lambda_offdiag=lambda_offdiag)
        self.closer = None
        if closing is not None:
            self.closer = closing.for_plan(self, recon_loss=recon_loss, alpha=alpha, beta=beta)
        self._build()
        if fuse_bn and training:
            # each BatchNorm finalisation carried by the call that produces its statistics
            # (vaehip.h bn_finalize).  The library runs it as its own launch right after the
            # producer: an in-kernel last-workgroup version measured 0.81 -> 1.26 ms/step (an
            # agent-scope release in every workgroup, and lower GEMM occupancy).
            self._fuse_finalize(self.fwd_calls)
            self._fuse_finalize(self.bwd_calls)
        # the backward as built, one call per op; bwd_calls batches its weight gradients
        # (batch_wgrads: one vae_conv_bwd_filter_batch per backward segment)
        self._bwd_raw = list(self.bwd_calls)
        self.batch_wgrads([len(self._bwd_raw)])

    def defer_reductions(self) -> bool:
        """Leave the step's weight-gradient slab reductions — the head backward's filter partials,
        the full-resolution ConvT backward's, the grouped weight gradients' K slices — and the loss
        fused into the head backward to the optimizer launch (vaehip.h defer_reduce,
        vae_adam_step_ex): three launches fewer per step.  For the one-rank fused step
        (engine.TrainStep), whose only reader of the gradients is its own Adam; each deferring call
        gets a workspace of its own, kept until the optimizer reads it.  bf16 training plans only;
        returns whether anything is.  A deferred plan stays so: backward() and a non-deferring TrainStep raise."""
        if self.deferred or self.net.dtype != torch.bfloat16 or not self.training:
            return self.deferred
        args = [a for fn, ref in self.bwd_calls if fn in (BATCH_FN, "vae_convT2d_bwd", "vae_head_bwd")
                for a in structs(ref)]
        for a in args:
            a.defer_reduce = 1
        if args:
            self.deferred = True
            self.size_workspaces()
        return self.deferred

    def batch_wgrads(self, ends):
        """Rebuild bwd_calls from bwd_calls_raw with the conv / convT weight gradients of each
        backward segment (calls [ends[k-1], ends[k]) of the raw list) moved into one
        vae_conv_bwd_filter_batch call at the segment's end, and size the workspaces.  Returns the
        segment ends as indices into the new list.  batch_wgrads=False (constructor) keeps one call
        per layer.

        With one segment (one rank) and wg_overlap, the decoder's weight gradients form a batch of
        their own, issued on the side stream where the decoder's data-gradient chain ends: it runs
        beside the encoder's data gradients (the critical path) instead of after them."""
        splits = []
        if self.wg_overlap and len(ends) == 1:
            raw = self.bwd_calls_raw
            # the decoder's backward ends where the bottleneck's begins (the fused latent kernels
            # or the latent Linear layers)
            first_lin = next((i for i, (fn, _) in enumerate(raw)
                              if fn in ("vae_latent_dec_bwd", "vae_linear_bwd_data")), None)
            if first_lin is not None:
                splits = [first_lin]
        if self.deterministic:
            for fn, ref in self.fwd_calls + self.bwd_calls_raw:
                for a in structs(ref):
                    if hasattr(a, "deterministic"):
                        a.deterministic = 1
        self.bwd_calls, new_ends = batch_filter_calls(self.bwd_calls_raw, ends, splits,
                                                      enabled=self.batch_wgrads_on)
        self.size_workspaces()
        return new_ends

    # ------------------------------------------------------------------ helpers
    def _bn_prod_bias(self, prefix: str) -> str:
        return prefix[:-2] + ".0.bias"          # "encoder.3.1" -> "encoder.3.0.bias"

    def bn_xf(self, prefix: str, kind: int, count: int, aux=None, running: bool = False,
              table: Optional[bool] = None) -> L.Xform:
        if table is None:
            table = not self.bn_in_consumer or self.wide_bn(prefix)
        net = self.net
        C = net.layout.bn_by_prefix[prefix].channels
        s = self.bnfwd[prefix]
        xf = L.Xform(kind=kind, channels=C, slope=SLOPE, count=float(count), eps=BN_EPS, momentum=BN_MOMENTUM)
        xf.sum, xf.sumsq, xf.reps, xf.rstride = s[0].data_ptr(), s[1].data_ptr(), s.shape[1], C
        xf.shift, xf.gamma, xf.beta = net.p(self._bn_prod_bias(prefix)), net.p(prefix + ".weight"), net.p(prefix + ".bias")
        if kind == L.X_BN_DY:
            xf.dgamma, xf.dbeta = self.bnbwd[prefix][0].data_ptr(), self.bnbwd[prefix][1].data_ptr()
        if table:
            xf.table = self.bntab[prefix].data_ptr() + (4 * 4 * C if kind == L.X_BN_DY else 0)
        if aux is not None:
            xf.aux = aux.data_ptr()
        if running:
            xf.running_mean, xf.running_var = net.run_stats(prefix)
        return xf

    def _publish(self, arg, xf, prefix: str):
        """Have a call write BatchNorm `prefix`'s dL/dgamma, dL/dbeta (through its BN_DY transform
        `xf`) and the closed-form bias gradient of the conv feeding it."""
        xf.dgamma_out, xf.dbeta_out = self.g(prefix + ".weight"), self.g(prefix + ".bias")
        arg.db = self.g(self._bn_prod_bias(prefix))

    def wide_bn(self, prefix: str) -> bool:
        """A BatchNorm wider than 512 channels (the Autoencoder's 1024-4096): its coefficient table is
        built once per step by vae_bn_finalize instead of in every consumer workgroup (the in-kernel
        build reduces <= 512 channels in one round of loads; wider ones would loop per channel in each
        of thousands of workgroups)."""
        return self.bn_in_consumer and self.net.layout.bn_by_prefix[prefix].channels > 512

    def fwd_sums(self, arg, prefix: str):
        """Producer side of a BatchNorm's forward statistics (conv / convT fwd epilogue)."""
        s = self.bnfwd[prefix]
        arg.y_sum, arg.y_sumsq = s[0].data_ptr(), s[1].data_ptr()
        arg.sum_reps, arg.sum_rstride = s.shape[1], s.shape[2]

    def bwd_sums(self, arg, prefix: str):
        """Producer side of a BatchNorm's backward sums (bwd_data epilogue of the next layer)."""
        s = self.bnbwd[prefix]
        arg.dx_dgamma, arg.dx_dbeta = s[0].data_ptr(), s[1].data_ptr()
        arg.sum_reps, arg.sum_rstride = s.shape[1], s.shape[2]

    def bwd_extras(self, arg, prefix: str):
        """bn_in_consumer: the weight-gradient call of the conv feeding BatchNorm `prefix` also
        publishes that BatchNorm's dL/dgamma, dL/dbeta and the conv's bias gradient (what
        vae_bn_finalize mode 1 did)."""
        if self.bn_in_consumer and not self.wide_bn(prefix):
            self._publish(arg, arg.dy_xf, prefix)

    def bn_finalize(self, lst, prefix: str, mode: int, count: int):
        """Queue vae_bn_finalize for one BatchNorm: mode 0 after the conv producing its input
        (table + running statistics), mode 1 after the kernel producing its backward sums
        (table + dγ, dβ + the producing conv's bias gradient in closed form)."""
        if self.bn_in_consumer and mode in (0, 1) and not self.wide_bn(prefix):
            return
        C = self.net.layout.bn_by_prefix[prefix].channels
        a = L.BnArgs(mode=mode)
        a.xf = self.bn_xf(prefix, L.X_BN_DY if mode == 1 else L.X_BN_ACT, count, running=(mode != 1), table=False)
        a.table = self.bntab[prefix].data_ptr() + (4 * 4 * C if mode == 1 else 0)
        if mode == 1:
            self._publish(a, a.xf, prefix)
        self._add(lst, "vae_bn_finalize", a)

    # ---- materialised transforms for the large layers (vaehip.h vae_bn_apply + vae_bgemm.hip)
    def big_layer(self, flops: float, cin: int, cout: int) -> bool:
        """A layer whose GEMMs take materialised (transform-free) operands: bf16 training, >= 4 GFLOP
        per pass and >= 128 channels on both sides (the Autoencoder's wide layers, whose GEMMs run on
        the 128 x 128 LDS-DMA tiles; the VanillaVAE's are 0.6 GFLOP, and IWAE's 32-channel final ConvT
        reaches 6 GFLOP at B*S = 320 but stays on its own kernels: materialised it measured 1.10 vs
        1.04 ms/step).  materialise=False keeps every transform fused into its consumers."""
        return (self.net.dtype == torch.bfloat16 and self.training and self.materialise
                and flops >= self.mat_min_flops and min(cin, cout) >= 128)

    def mat_act(self, F, prefix: str, t: torch.Tensor):
        """lrelu(BN(t)) written once (vae_bn_apply: running statistics updated there, the forward's
        first consumer of the BatchNorm) into _mat_a[prefix], which every later consumer reads plainly
        (_read)."""
        out = self._mat_a[prefix] = torch.empty_like(t)
        a = L.BnApplyArgs(dtype=self.net.dcode, rows=t.numel() // t.shape[-1], channels=t.shape[-1])
        a.x, a.out = t.data_ptr(), out.data_ptr()
        a.xf = self.bn_xf(prefix, L.X_BN_ACT, _cnt(t), running=True)
        self._add(F, "vae_bn_apply", a)

    def mat_dz(self, Bw, prefix: str, g: torch.Tensor, y: torch.Tensor):
        """The BatchNorm-backward gradient A g + B y + C of a big layer's output written once
        (vae_bn_apply BN_DY, which also publishes dgamma, dbeta and the conv's closed-form bias
        gradient unless vae_bn_finalize did); the layer's data and weight gradients read it plainly."""
        out = self._mat_dz[prefix] = torch.empty_like(g)
        a = L.BnApplyArgs(dtype=self.net.dcode, rows=g.numel() // g.shape[-1], channels=g.shape[-1])
        a.x, a.out = g.data_ptr(), out.data_ptr()
        a.xf = self.bn_xf(prefix, L.X_BN_DY, _cnt(y), aux=y)
        if self.bn_in_consumer and not self.wide_bn(prefix):
            self._publish(a, a.xf, prefix)
        self._add(Bw, "vae_bn_apply", a)
        return out

    def _read(self, a, prefix: str, t: torch.Tensor, running: bool = False):
        """A call's x operand lrelu(BN(t)): the materialised copy (mat_act), else t transformed on load."""
        if prefix in self._mat_a:
            a.x = self._mat_a[prefix].data_ptr()
        else:
            a.x, a.x_xf = t.data_ptr(), self.bn_xf(prefix, L.X_BN_ACT, _cnt(t), running=running)

    def _bwd_dy(self, Bw, prefix: str, g: torch.Tensor, y: torch.Tensor, big: bool):
        """The dy operand of a layer's backward calls from the stored gradient g of its output y:
        (pointer, transform, materialised) — mat_dz for a big layer, else BN backward on load."""
        self.bn_finalize(Bw, prefix, 1, _cnt(y))
        if big:
            return self.mat_dz(Bw, prefix, g, y).data_ptr(), L.Xform(kind=L.X_NONE, channels=y.shape[-1]), True
        return g.data_ptr(), self.bn_xf(prefix, L.X_BN_DY, _cnt(y), aux=y), False

    def _fuse_finalize(self, calls):
        """Fold every vae_bn_finalize call (modes 0/1) into the call that produced its statistics
        (the GEMM whose epilogue wrote them): that call's last workgroup then builds the table
        (vaehip.h bn_finalize), saving a dependent launch per BatchNorm and direction."""
        out = []
        nctr = 0
        for fn, ref in calls:
            bn = structs(ref)[0] if fn == "vae_bn_finalize" else None
            if bn is not None and bn.mode in (0, 1):
                field, key = ("y_sum", bn.xf.sum) if bn.mode == 0 else ("dx_dgamma", bn.xf.dgamma)
                prod = next((a for _, pref in reversed(out) for a in structs(pref)
                             if hasattr(a, "bn_counter") and getattr(a, field, None) == key), None)
                if prod is not None and not prod.bn_finalize:
                    prod.bn_finalize = ctypes.pointer(bn)
                    prod.bn_counter = self.counters.data_ptr() + 4 * nctr
                    nctr += 1
                    continue
            out.append((fn, ref))
        calls[:] = out

    def _conv(self, n: int, sp: int, cin: int, cout: int, out: int, stride: int = 2) -> L.ConvArgs:
        """ConvArgs of a 3x3 pad-1 layer from an sp x sp to an out x out map (forward orientation)."""
        return L.ConvArgs(dtype=self.net.dcode, n=n, h=sp, w=sp, c=cin, k=cout, p=out, q=out, r=3, stride=stride, pad=1)

    # ------------------------------------------------------------------ plan
    def _build(self):
        n = len(self.net.hidden_dims)
        self._enc_pre = [f"encoder.{i}.1" for i in range(n)]
        self._dec_pre = [f"decoder.{i}.1" for i in range(n - 1)] + ["final_layer.1"]
        self._dec_w = [f"decoder.{i}.0" for i in range(n - 1)] + ["final_layer.0"]
        self._dec_out, self._g_dec_out = self.dec + [self.fin], self.g_dec + [self.g_fin]
        for stage in (self._fwd_encoder, self._fwd_bottleneck, self._fwd_decoder, self._fwd_head_loss):
            stage(self.fwd_calls)
        if self.training:
            for stage in (self._bwd_head, self._bwd_decoder, self._bwd_bottleneck, self._bwd_encoder):
                stage(self.bwd_calls)

    def _fwd_encoder(self, F):
        """The step's padding calls (image, first-layer and wide-head weights), then the encoder convs."""
        net, T, B, img = self.net, self.net.dcode, self.B, self.net.img_size
        h, enc_pre = net.hidden_dims, self._enc_pre
        fmode = 0 if self.training else 2            # bn_finalize: batch statistics / running statistics
        if self.pad_rgb:
            F.append(("vae_nchw_to_nhwc_pad", (T, B, 3, img, img, 8, self.x.data_ptr(), self.x8.data_ptr())))
            F.append(("vae_pad_channels", (T, h[0] * 9, 3, 8, net.w("encoder.0.0.weight"), self.w8.data_ptr())))
        if self.wide_head:          # head weights [3][3][3][C] -> [8][3][3][C] (one row of 27C -> 72C)
            F.append(("vae_pad_channels", (T, 1, 27 * h[0], 72 * h[0], net.w("final_layer.3.weight"), self.w8h.data_ptr())))
            # the GEMM epilogue reads 8 bias values (its N): pad the 3-element bias too
            F.append(("vae_pad_channels", (L.F32, 1, 3, 8, net.p("final_layer.3.bias"), self.b8h.data_ptr())))
        sp = img
        for i in range(len(h)):
            a = self._conv(B, sp, 3 if i == 0 else h[i - 1], h[i], sp // 2)
            if i == 0 and self.pad_rgb:
                a.c, a.x = 8, self.x8.data_ptr()
            elif i == 0:
                a.x_nchw_f32, a.x = 1, self.x.data_ptr()
            else:
                if self.big_layer(2.0 * B * (sp // 2) ** 2 * h[i] * 9 * h[i - 1], h[i - 1], h[i]):
                    self.mat_act(F, enc_pre[i - 1], self.enc[i - 1])
                self._read(a, enc_pre[i - 1], self.enc[i - 1], running=True)
            a.wt = self.w8.data_ptr() if (i == 0 and self.pad_rgb) else net.w(f"encoder.{i}.0.weight")
            a.bias, a.y = net.p(f"encoder.{i}.0.bias"), self.enc[i].data_ptr()
            if self.training:
                self.fwd_sums(a, enc_pre[i])
            self._add(F, "vae_conv2d_fwd", a)
            self.bn_finalize(F, enc_pre[i], fmode, _cnt(self.enc[i]))
            sp //= 2

    def _fwd_bottleneck(self, F):
        """fc_mu|fc_var, the reparameterization [and InfoVAE's MMD] and decoder_input: two
        vae_latent_* launches (latent_fused) or one call per op.  Sets n_encode / n_decode0."""
        net, T, B, BS = self.net, self.net.dcode, self.B, self.B * self.S
        D, C5, r0 = net.latent_dim, net.hidden_dims[-1], net.hidden_dims[-1]
        last, pre = self.enc[-1], self._enc_pre[-1]
        if self.latent_fused:
            la = self._latent = L.LatentArgs(dtype=T, batch=B, samples=self.S, latent=D, in_features=4 * C5,
                                              out_features=4 * r0)
            la.x, la.x_xf = last.data_ptr(), self.bn_xf(pre, L.X_BN_ACT, _cnt(last), running=True)
            la.w1, la.b1 = net.w("fc_mu.weight"), net.p("fc_mu.bias")
            la.mulv, la.eps, la.z = self.mulv.data_ptr(), self.eps.data_ptr(), self.z.data_ptr()
            la.w2, la.b2, la.h = net.w("decoder_input.weight"), net.p("decoder_input.bias"), self.h0.data_ptr()
            self._add(F, "vae_latent_fc_fwd", la)
            self.n_encode = self.n_decode0 = len(F)     # (decode() of a fused plan starts at the reparameterization)
            F.append(("vae_latent_dec_fwd", F[-1][1]))
            if self.term is not None:          # (behind the kernel that draws / reads this step's eps)
                self.term.queue(F)
            return
        a = L.LinearArgs(dtype=T, m=B, n=2 * D, k=4 * C5)
        a.x, a.x_xf = last.data_ptr(), self.bn_xf(pre, L.X_BN_ACT, _cnt(last), running=True)
        a.wt, a.bias = net.w("fc_mu.weight"), net.p("fc_mu.bias")
        a.y, a.y_f32 = self.mulv.data_ptr(), 1
        self._add(F, "vae_linear_fwd", a)
        self.n_encode = len(F)             # calls of encode(): encoder + fc_mu|fc_var
        F.append(("vae_reparam_fwd", (T, BS, self.S, D, self.mulv.data_ptr(), self.eps.data_ptr(), self.z.data_ptr())))
        if self.term is not None:
            self.term.queue(F)
        self.n_decode0 = len(F)            # decode(): decoder_input .. head
        a = L.LinearArgs(dtype=T, m=BS, n=4 * r0, k=D)
        a.x, a.y = self.z.data_ptr(), self.h0.data_ptr()
        a.wt, a.bias = net.w("decoder_input.weight"), net.p("decoder_input.bias")
        self._add(F, "vae_linear_fwd", a)

    def _dec_shape(self, i: int):
        """(input spatial size, input channels, output channels) of the decoder's i-th ConvTranspose2d."""
        r = self.net.hidden_dims[::-1]
        return 2 * 2 ** i, r[i], r[min(i + 1, len(r) - 1)]

    def _fwd_decoder(self, F):
        net, BS = self.net, self.B * self.S
        fmode = 0 if self.training else 2
        prev, prev_pre = self.h0, None
        for i, (out, pre, w) in enumerate(zip(self._dec_out, self._dec_pre, self._dec_w)):
            sp, cin, cout = self._dec_shape(i)
            a = self._conv(BS, sp, cin, cout, 2 * sp)
            if prev_pre is None:
                a.x = prev.data_ptr()
            else:
                if self.big_layer(2.0 * BS * sp * sp * cin * cout * 9, cin, cout):
                    self.mat_act(F, prev_pre, prev)
                self._read(a, prev_pre, prev, running=True)
            a.wt, a.wt_t = net.w(w + ".weight"), net.wt_t.get(w + ".weight")
            a.bias, a.y = net.p(w + ".bias"), out.data_ptr()
            if self.training:
                self.fwd_sums(a, pre)
            self._add(F, "vae_convT2d_fwd", a)
            self.bn_finalize(F, pre, fmode, _cnt(out))
            prev, prev_pre = out, pre

    def _head_args(self, running: bool) -> L.HeadArgs:
        """What vae_head_fwd and vae_head_bwd share: input (final BN+LeakyReLU on load), weights, target, recon."""
        net, img = self.net, self.net.img_size
        hd = L.HeadArgs(dtype=net.dcode, n=self.B * self.S, h=img, w=img, c=self.fin.shape[-1], samples=self.S)
        hd.x, hd.x_xf = self.fin.data_ptr(), self.bn_xf("final_layer.1", L.X_BN_ACT, _cnt(self.fin), running=running)
        hd.wt, hd.bias = net.p("final_layer.3.weight"), net.p("final_layer.3.bias")
        hd.target, hd.recon = self.x.data_ptr(), self.recon.data_ptr()
        return hd

    def _fwd_head_loss(self, F):
        """The head (tanh, reconstruction, per-image SSE) and the loss that closes the forward.  Sets
        n_decode1, elbo_args and elbo_in_head."""
        T, B, img = self.net.dcode, self.B, self.net.img_size
        if self.wide_head:
            self._wide_head_fwd(F)
        else:
            hd = self._head_args(running=True)
            hd.sse = self.sse.data_ptr()
            self._add(F, "vae_head_fwd", hd)
        e = L.ElboArgs(kind=self.loss_kind, batch=B, samples=self.S, latent=self.net.latent_dim, img_elems=3 * img * img,
                       kld_weight=self.kld_weight, beta=self.beta, gamma=self.gamma, c_max=self.max_capacity,
                       c_stop_iter=self.capacity_max_iter)
        e.iter, e.mulv, e.sse = self.num_iter.data_ptr(), self.mulv.data_ptr(), self.sse.data_ptr()
        e.out, e.per_img = self.out.data_ptr(), self.per_img.data_ptr()
        e.head_coef, e.kl_coef = self.head_coef.data_ptr(), self.kl_coef.data_ptr()
        if self.term is not None:
            self.term.fill_elbo(e)
        if self.loss_kind == L.LOSS_MIWAE:  # (VAE_LOSS_MIWAE: the tile count is its estimates M)
            e.mmd_tiles = self.M
        self.n_decode1, self.elbo_args = len(F), e
        # elbo_in_head: the loss evaluated by the head backward (vaehip.h vae_head_args.elbo: one
        # extra workgroup of its filter-partial reduction, the seed coefficient a constant) instead
        # of a vae_elbo_fwd launch between the forward and the backward — the bf16 head kernels,
        # the vanilla / BetaVAE-H losses (their seeds do not depend on the batch), one sample
        self.elbo_in_head = (self.fused_loss and self.training and self.closer is None and not self.wide_head
                             and self.S == 1 and T == L.BF16 and B <= 1024
                             and self.loss_kind in (L.LOSS_VANILLA, L.LOSS_BETA_H))
        # (with elbo_in_head, out / per_img / head_coef / kl_coef are written by the backward: they
        # are this step's only after backward() — loss_dict() raises in between)
        if self.closer is not None:
            self.closer.join(self, F)
        elif self.fused_loss and not self.elbo_in_head and self.loss not in CLOSERS:
            # (an eval plan of a loss in CLOSERS has no loss call: its loss is the caller's, never the ELBO's)
            self._add(F, "vae_elbo_fwd", e)

    def _bwd_head(self, Bw):
        self._head_bwd = None            # (wide head: its seed is vae_recon_bwd's; seed_fused)
        if self.wide_head:
            return self._wide_head_bwd(Bw)
        hb = self._head_bwd = self._head_args(running=False)
        if self.seed_recon:
            hb.grad_recon = self.grad_recon.data_ptr()
        else:
            hb.coef = self.head_coef.data_ptr()
        hb.dx, hb.dx_epi = self.g_fin.data_ptr(), self.bn_xf("final_layer.1", L.X_BN_ACT, _cnt(self.fin), aux=self.fin)
        self.bwd_sums(hb, "final_layer.1")
        hb.dw, hb.db = self.g("final_layer.3.weight"), self.g("final_layer.3.bias")
        if self.elbo_in_head:
            hb.elbo = ctypes.addressof(self.elbo_args)
        self._add(Bw, "vae_head_bwd", hb)

    def _bwd_decoder(self, Bw):
        """The ConvTranspose2d blocks, last first: data gradient into the previous BatchNorm's
        backward epilogue and weight gradient, each reading dy through this block's BN backward."""
        net, BS, nd = self.net, self.B * self.S, len(self._dec_out)
        dec_out, g_dec_out, dec_pre, dec_w = self._dec_out, self._g_dec_out, self._dec_pre, self._dec_w
        for i in reversed(range(nd)):
            sp, cin, cout = self._dec_shape(i)
            x_t = self.h0 if i == 0 else dec_out[i - 1]
            gx_t = self.g_h0 if i == 0 else g_dec_out[i - 1]
            dy, dy_xf, mat = self._bwd_dy(Bw, dec_pre[i], g_dec_out[i], dec_out[i],
                                          self.big_layer(2.0 * BS * sp * sp * cin * cout * 9, cin, cout))
            a = self._conv(BS, sp, cin, cout, 2 * sp)
            a.dy, a.dy_xf = dy, dy_xf
            a.wt, a.dx = net.w(dec_w[i] + ".weight"), gx_t.data_ptr()
            if i > 0:
                a.dx_epi = self.bn_xf(dec_pre[i - 1], L.X_BN_ACT, _cnt(x_t), aux=x_t)
                self.bwd_sums(a, dec_pre[i - 1])
            # the full-resolution last ConvTranspose2d: both gradients in one pass over dy
            # (vaehip.h vae_convT2d_bwd; other shapes run the two calls inside it)
            f = a if i == nd - 1 else self._conv(BS, sp, cin, cout, 2 * sp)
            if i == 0:
                f.x = x_t.data_ptr()
            else:
                self._read(f, dec_pre[i - 1], x_t)
            f.dy, f.dy_xf = dy, dy_xf
            f.dw = self.g(dec_w[i] + ".weight")      # bias gradient: closed form (bn_finalize / bwd_extras)
            if not mat:
                self.bwd_extras(f, dec_pre[i])
            if f is a:
                self._add(Bw, "vae_convT2d_bwd", a)
            else:
                self._add(Bw, "vae_convT2d_bwd_data", a)
                self._add(Bw, "vae_convT2d_bwd_filter", f)

    def _bwd_bottleneck(self, Bw):
        """decoder_input and fc_mu|fc_var backwards around the reparameterization + KL gradient."""
        net, T, B, BS = self.net, self.net.dcode, self.B, self.B * self.S
        D, C5, r0 = net.latent_dim, net.hidden_dims[-1], net.hidden_dims[-1]
        last, g_last, pre = self.enc[-1], self.g_enc[-1], self._enc_pre[-1]
        self._reparam_bwd = None
        if self.latent_fused:
            la = self._latent
            la.dh, la.kl_coef, la.dmulv = self.g_h0.data_ptr(), self.kl_coef.data_ptr(), self.dmulv.data_ptr()
            la.dw2, la.db2 = self.g("decoder_input.weight"), self.g("decoder_input.bias")
            la.dx, la.dx_epi = g_last.data_ptr(), self.bn_xf(pre, L.X_BN_ACT, _cnt(last), aux=last)
            self.bwd_sums(la, pre)
            la.dw1, la.db1 = self.g("fc_mu.weight"), self.g("fc_mu.bias")
            Bw += [(fn, self.fwd_calls[self.n_encode - 1][1]) for fn in ("vae_latent_dec_bwd", "vae_latent_fc_bwd")]
            return
        # decoder_input: dz -> d[mu|logvar] (reparameterization + KL), and its weight grads
        a = self._reparam_bwd = L.LinearArgs(dtype=T, m=BS, n=4 * r0, k=D)
        a.dy, a.wt = self.g_h0.data_ptr(), net.w("decoder_input.weight")
        a.mulv, a.eps, a.dmulv, a.samples = self.mulv.data_ptr(), self.eps.data_ptr(), self.dmulv.data_ptr(), self.S
        a.kl_coef = self.kl_coef.data_ptr() if self.fused_loss else None
        self._add(Bw, "vae_linear_bwd_data", a)
        f = L.LinearArgs(dtype=T, m=BS, n=4 * r0, k=D)
        f.dy, f.x = self.g_h0.data_ptr(), self.z.data_ptr()
        f.dw, f.db = self.g("decoder_input.weight"), self.g("decoder_input.bias")
        self._add(Bw, "vae_linear_bwd_filter", f)
        # fc_mu | fc_var
        a = L.LinearArgs(dtype=T, m=B, n=2 * D, k=4 * C5)
        a.dy, a.dy_f32, a.wt = self.dmulv.data_ptr(), 1, net.w("fc_mu.weight")
        a.dx, a.dx_epi = g_last.data_ptr(), self.bn_xf(pre, L.X_BN_ACT, _cnt(last), aux=last)
        self.bwd_sums(a, pre)
        self._add(Bw, "vae_linear_bwd_data", a)
        f = L.LinearArgs(dtype=T, m=B, n=2 * D, k=4 * C5)
        f.dy, f.dy_f32 = self.dmulv.data_ptr(), 1
        f.x, f.x_xf = last.data_ptr(), self.bn_xf(pre, L.X_BN_ACT, _cnt(last))
        f.dw, f.db = self.g("fc_mu.weight"), self.g("fc_mu.bias")
        self._add(Bw, "vae_linear_bwd_filter", f)

    def _bwd_encoder(self, Bw):
        """The encoder convs, last first: weight gradient, then (blocks 1..) the data gradient."""
        net, B, h, enc_pre = self.net, self.B, self.net.hidden_dims, self._enc_pre
        for i in reversed(range(len(h))):
            sp = net.img_size // 2 ** i
            cin = 3 if i == 0 else h[i - 1]
            dy, dy_xf, mat = self._bwd_dy(Bw, enc_pre[i], self.g_enc[i], self.enc[i], i > 0 and self.big_layer(
                2.0 * B * (sp // 2) ** 2 * h[i] * 9 * cin, cin, h[i]))
            f = self._conv(B, sp, cin, h[i], sp // 2)
            f.dy, f.dy_xf = dy, dy_xf
            f.dw = self.g(f"encoder.{i}.0.weight")       # bias gradient: closed form (bn_finalize / bwd_extras)
            if i == 0 and self.pad_rgb:
                # the 8-channel padded image; dW lands in the parameter's own [k][3][3][3] layout
                # (vaehip.h dw_inner: the weight-gradient GEMM drops the pad channels)
                f.c, f.x, f.dw_inner = 8, self.x8.data_ptr(), 3
            elif i == 0:
                f.x_nchw_f32, f.x = 1, self.x.data_ptr()
            else:
                self._read(f, enc_pre[i - 1], self.enc[i - 1])
            if not mat:
                self.bwd_extras(f, enc_pre[i])
            self._add(Bw, "vae_conv2d_bwd_filter", f)
            if i > 0:
                a = self._conv(B, sp, cin, h[i], sp // 2)
                a.dy, a.dy_xf = dy, dy_xf
                a.wt, a.wt_t = net.w(f"encoder.{i}.0.weight"), net.wt_t.get(f"encoder.{i}.0.weight")
                a.dx = self.g_enc[i - 1].data_ptr()
                a.dx_epi = self.bn_xf(enc_pre[i - 1], L.X_BN_ACT, _cnt(self.enc[i - 1]), aux=self.enc[i - 1])
                self.bwd_sums(a, enc_pre[i - 1])
                self._add(Bw, "vae_conv2d_bwd_data", a)

    def _wide_head_fwd(self, F):
        """Head of a final layer wider than 32 channels: Conv2d(C -> 3 padded to 8, k3 s1 p1) on the
        conv-GEMM path with BatchNorm+LeakyReLU applied to its input on load, then vae_recon_fwd:
        tanh -> NCHW reconstruction, per-image SSE, and with the fused loss the backward seed
        dL/dy = 2(recon - x)(1 - recon^2) / (B*3*H*W) (the mean-MSE term of the ELBO)."""
        T, img, BS = self.net.dcode, self.net.img_size, self.B * self.S
        C = self.fin.shape[-1]
        a = self._conv(BS, img, C, 8, img, stride=1)
        a.x, a.x_xf = self.fin.data_ptr(), self.bn_xf("final_layer.1", L.X_BN_ACT, _cnt(self.fin), running=True)
        a.wt, a.bias, a.y = self.w8h.data_ptr(), self.b8h.data_ptr(), self.y8.data_ptr()    # (y8[..., 3:] is never read)
        self._add(F, "vae_conv2d_fwd", a)
        rc = L.ReconArgs(dtype=T, n=BS, h=img, w=img, c=3, ld=8)
        rc.y, rc.target, rc.recon, rc.sse = self.y8.data_ptr(), self.x.data_ptr(), self.recon.data_ptr(), self.sse.data_ptr()
        if self.fused_loss and self.training and self.closer is None:
            # (DIP-VAE's reconstruction term is the sum, dip_vae.py:141: no 1/(B*3*H*W))
            rc.dy = self.g8.data_ptr()
            recon_sum = self.term is not None and self.term.recon_sum
            rc.grad_scale = 1.0 if recon_sum else 1.0 / (self.B * 3 * img * img)
        self._add(F, "vae_recon_fwd", rc)

    def _wide_head_bwd(self, Bw):
        """Backward of _wide_head_fwd: [the seed from dL/drecon (drop-in)], data gradient into the final
        BatchNorm+LeakyReLU backward epilogue (its Σg, Σg·x̂), weight / bias gradient of the padded
        head, and the padded gradients' first 3 rows added into the parameter gradients."""
        T, img, BS = self.net.dcode, self.net.img_size, self.B * self.S
        C = self.fin.shape[-1]
        if self.seed_recon:
            rb = L.ReconArgs(dtype=T, n=BS, h=img, w=img, c=3, ld=8)
            rb.target, rb.recon = self.x.data_ptr(), self.recon.data_ptr()
            rb.dy, rb.grad_recon = self.g8.data_ptr(), self.grad_recon.data_ptr()
            self._add(Bw, "vae_recon_bwd", rb)
        a = self._conv(BS, img, C, 8, img, stride=1)
        a.dy, a.wt = self.g8.data_ptr(), self.w8h.data_ptr()
        a.dx, a.dx_epi = self.g_fin.data_ptr(), self.bn_xf("final_layer.1", L.X_BN_ACT, _cnt(self.fin), aux=self.fin)
        self.bwd_sums(a, "final_layer.1")
        self._add(Bw, "vae_conv2d_bwd_data", a)
        f = self._conv(BS, img, C, 8, img, stride=1)
        f.dy = self.g8.data_ptr()
        f.x, f.x_xf = self.fin.data_ptr(), self.bn_xf("final_layer.1", L.X_BN_ACT, _cnt(self.fin))
        f.dw, f.db = self.dw8h.data_ptr(), self.db8h.data_ptr()
        self._add(Bw, "vae_conv2d_bwd_filter", f)
        Bw.append(("vae_unpad_accumulate", (1, 72 * C, 27 * C, self.dw8h.data_ptr(), self.g("final_layer.3.weight"))))
        Bw.append(("vae_unpad_accumulate", (1, 8, 3, self.db8h.data_ptr(), self.g("final_layer.3.bias"))))

    def use_device_eps(self, step: torch.Tensor, seed: int = 1265) -> bool:
        """Draw eps ~ N(0,1) on the device inside the forward, every step (the reference's
        torch.randn_like(std), vanilla_vae.py:116): vae_latent_dec_fwd runs Philox4x32-10 keyed by
        `seed` with the device step counter `step` (int32, advanced by vae_step_begin[_ex]) and writes
        the draw to self.eps for the backward.  Only the fused bf16 bottleneck (latent_fused) draws;
        returns False (eps stays an input) otherwise."""
        if not self.latent_fused:
            return False
        la = self._latent
        la.eps_gen, la.eps_step, la.eps_seed = 1, step.data_ptr(), seed & 0xFFFFFFFFFFFFFFFF
        self._eps_step = step                       # keep the counter alive with the plan
        return True

    def use_device_prior(self, step: torch.Tensor, seed: int = 1265) -> bool:
        """Have the latent term draw its prior sample (self.prior) on the device, every step
        (MmdTerm.use_device_prior); returns False for a plan whose loss has no such input."""
        return self.prior is not None and self.term.use_device_prior(step, seed)

    @property
    def prior(self):
        return self.term.prior if self.term is not None else None

    def draw_noise(self, eps: bool = True, prior: bool = True):
        if eps:
            self.eps.normal_()                        # torch.randn_like(std), vanilla_vae.py:116
        if prior and self.prior is not None:
            self.prior.normal_()                      # torch.randn_like(z), info_vae.py:220

    # ------------------------------------------------------------------ execution
    def begin(self, stream=None):
        super().begin(stream)
        if self.loss_kind == L.LOSS_BETA_B:
            self.num_iter.add_(1.0)

    def loss_dict(self) -> Dict[str, float]:
        if self._loss_pending:
            raise RuntimeError("loss_dict(): this plan evaluates the ELBO in the head backward "
                               "(elbo_in_head); run backward() first")
        d = super().loss_dict()
        if self.term is not None:
            self.term.place(d, float(self.term.value))
        return d

    @property
    def extra_term(self):
        """(name, one-element tensor) of the loss dict's fourth entry, for the losses with a
        batch-coupled latent term (InfoVAE's MMD, DIP-VAE's DIP_Loss); None otherwise."""
        return (self.term.name, self.term.value) if self.term is not None else None

    # the earlier spellings of the term's buffers, which the step tests read: the MMD's dmmd/dz and
    # DIP-VAE's d dip/d[mu | log_var] (term.grad), the dip value (term.value; None without a term)
    dz_mmd = dmulv_dip = property(lambda self: self.term.grad)
    dip = property(lambda self: self.term.value if self.term is not None else None)

    # ------------------------------------------------------------------ drop-in ELBO
    # A drop-in plan (fused_loss=False) can still take its loss on the GPU: the BaseVAE
    # loss_function of vae_amd.models runs vae_elbo_fwd on the forward's own buffers (run_elbo)
    # and seeds the backward from the kernel's coefficients (seed_fused) instead of autograd's
    # dL/drecon and dL/d[mu|log_var].
    LOSS_KINDS = {"vanilla": L.LOSS_VANILLA, "betaH": L.LOSS_BETA_H, "betaB": L.LOSS_BETA_B,
                  "iwae": L.LOSS_IWAE, "info": L.LOSS_INFO, "dip": L.LOSS_DIP, "miwae": L.LOSS_MIWAE,
                  # (a loss in CLOSERS has no vae_loss_kind: its drop-in plan and its eval plan are the
                  # vanilla ones)
                  **{name: L.LOSS_VANILLA for name in CLOSERS}}

    def run_elbo(self, stream, loss: str, kld_weight: float, beta: float = 4.0, gamma: float = 1000.0,
                 max_capacity: float = 25.0, capacity_max_iter: float = 1e5, num_iter: Optional[int] = None,
                 alpha: float = -0.5, reg_weight: float = 100.0, prior: Optional[torch.Tensor] = None,
                 c_max: Optional[float] = None, c_stop_iter: Optional[float] = None):
        """vae_elbo_fwd over this step's SSE and mu|log_var: out = [loss, Reconstruction_Loss, KLD
        as the reference reports it, raw KLD]; per_img; head_coef / kl_coef = dloss/dsse_i and the
        per-row KL gradient coefficient (the backward seeds).  The loss arguments are spelled as the
        constructor's; c_max / c_stop_iter are the older names of max_capacity / capacity_max_iter."""
        if loss in CLOSERS:
            raise ValueError(f"run_elbo({loss!r}): this loss runs on {CLOSERS[loss].fn} (StepPlan(loss={loss!r}), "
                             f"the model's loss_function), not on the ELBO kernel")
        e = self.elbo_args
        e.kind = self.LOSS_KINDS[loss]
        if e.kind == L.LOSS_MIWAE:
            # (M*K rows per image in b, m, k order; M = K = 1 is the plain ELBO on one sample)
            if self.loss_kind != L.LOSS_MIWAE:
                raise ValueError("run_elbo('miwae') needs a plan built with loss='miwae'")
            e.mmd_tiles = self.M
        elif (e.kind == L.LOSS_IWAE) != (self.S > 1):
            raise ValueError(f"loss {loss!r} on a plan with {self.S} samples per image")
        e.kld_weight, e.beta, e.gamma = kld_weight, beta, gamma
        e.c_max = max_capacity if c_max is None else c_max
        e.c_stop_iter = capacity_max_iter if c_stop_iter is None else c_stop_iter
        if num_iter is not None:
            self.num_iter.fill_(float(num_iter))
        if loss in TERMS:
            # the term of this forward's latents: its unscaled gradient and the partials the loss adds
            if not isinstance(self.term, TERMS[loss]) or self.fused_loss:
                raise ValueError(f"run_elbo({loss!r}) needs a drop-in plan built with loss={loss!r}")
            self.term.run(e, stream, beta=beta, alpha=alpha, reg_weight=reg_weight, prior=prior)
        L.call("vae_elbo_fwd", e, stream)

    def seed_fused(self, on: bool):
        """Backward seeding of a drop-in plan: on — from head_coef / kl_coef (run_elbo); off — from
        grad_recon and dmulv as written by autograd (the caller's own loss)."""
        if self.fused_loss or not self.training:
            return
        hb, rb = self._head_bwd, self._reparam_bwd
        if hb is None:               # wide head: its seed is vae_recon_bwd's, from grad_recon
            if on:                   # dL/drecon of the GPU ELBO: head_coef[n] * (recon - x)
                S = self.S
                torch.mul(self.head_coef.view(-1, 1, 1, 1),
                          self.recon - self.x.repeat_interleave(S, 0) if S > 1 else self.recon - self.x,
                          out=self.grad_recon)
                rb.kl_coef = self.kl_coef.data_ptr()
            else:
                rb.kl_coef = None
            return
        if on:
            hb.coef, hb.grad_recon = self.head_coef.data_ptr(), None
            rb.kl_coef = self.kl_coef.data_ptr()
        else:
            hb.coef, hb.grad_recon = None, self.grad_recon.data_ptr()
            rb.kl_coef = None

    def reset_backward(self):
        """Zero what the backward accumulates (gradients, BatchNorm-backward sums, d[mu|logvar],
        the padded head's dW) so the backward of the same forward can run again."""
        self.grads.zero_()
        for t in self.bnbwd.values():
            t.zero_()
        self.dmulv.zero_()
        if self.wide_head:
            self.dw8h.zero_()
            self.db8h.zero_()


def bn_reps(channels: int) -> int:
    """Replicas of a BatchNorm's statistics: enough that the ~1000 workgroups of a producing
    kernel do not all add into the same 2*C addresses, few enough (reps*C <= 256: one element per
    thread per statistic) that every consuming workgroup reduces them in one round of loads
    (vae_common.hpp tab_build) — thousands of consumer workgroups re-read them."""
    return max(1, min(32, 256 // max(1, channels)))


def _cnt(t: torch.Tensor) -> int:
    """BatchNorm reduction size of a stored NHWC map."""
    return t.shape[0] * t.shape[1] * t.shape[2]
