"""What every network and every step plan is built on: `NetBase` (flat parameters, their bf16 and
swapped-axes copies), `PlanBase` (the contract engine.TrainStep, dp and experiment.GraphedSteps rely
on, with the code the plans share) and `ZeroRegion` (the layout of the buffer the step head clears)."""
from __future__ import annotations

import ctypes
from typing import Dict, List

import torch

from . import _lib as L
from .calls import run_calls, size_workspaces
from .layout import Layout, default_init


def _pad4(n: int) -> int:
    return (n + 3) // 4 * 4


class NetBase:
    """Flat fp32 parameters of a network on one device in native layouts (layout.py), their bf16
    copy for the GEMMs (bf16 mode) and the swapped-axes copies of the weights read transposed."""

    # whether a TrainStep's head launch refreshes the swapped copies itself (engine.begin_args):
    # a net whose copies fit one vae_swap_axes descriptor array; else its own launches (refresh_swaps)
    swaps_in_step_begin = False

    def __init__(self, layout: Layout, ref_order, dtype: torch.dtype, device, generator):
        self.layout, self.ref_order, self.dtype = layout, ref_order, dtype
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        cpu_p = torch.zeros(layout.total)
        cpu_r = torch.zeros(max(1, layout.bn_total))          # (one unused element without BatchNorm)
        default_init(layout, cpu_p, cpu_r[:layout.bn_total], generator)
        self.params = cpu_p.to(self.device)
        self.running = cpu_r.to(self.device)
        self.lowp = (torch.zeros(layout.total, dtype=torch.bfloat16, device=self.device)
                     if dtype == torch.bfloat16 else None)
        self.num_batches_tracked = 0
        self.wt_t: Dict[str, int] = {}      # parameter name -> device pointer of its swapped copy
        self.swap_descs: List = []          # vae_swap_axes descriptor arrays (<= SWAP_MAX each)
        self.swaps_stale = False            # the swapped copies trail the parameters (FusedAdam.apply)

    @property
    def dcode(self) -> int:
        return L.dtype_code(self.dtype)

    def refresh_swaps(self, stream=None):
        self.swaps_stale = False
        for d in self.swap_descs:
            L.call("vae_swap_axes", len(d), ctypes.byref(d), stream if stream is not None else L.stream_ptr())

    def sync_lowp(self):
        """Refresh the bf16 weight copy from the fp32 master (bf16 mode only)."""
        if self.lowp is not None:
            L.call("vae_cast_bf16", self.params.numel(), self.params.data_ptr(), self.lowp.data_ptr(), L.stream_ptr())
            self.refresh_swaps()

    def load_reference_state_dict(self, sd: Dict[str, torch.Tensor]):
        self.layout.load_reference(self.params, self.running, {k: v.to(self.device) for k, v in sd.items()})
        bns = self.layout.bns
        nbt = sd.get(bns[0].prefix + ".num_batches_tracked") if bns else None
        self.num_batches_tracked = int(nbt) if nbt is not None else 0
        self.sync_lowp()

    def reference_state_dict(self) -> Dict[str, torch.Tensor]:
        return self.layout.export_reference(self.params, self.running, self.num_batches_tracked, self.ref_order)

    # ------------------------------------------------------------------ pointers
    def p(self, name: str) -> int:
        """fp32 master pointer of a parameter."""
        s = self.layout.by_name[name]
        return self.params.data_ptr() + 4 * s.offset

    def w(self, name: str) -> int:
        """Pointer of the copy a GEMM reads (bf16 in bf16 mode)."""
        s = self.layout.by_name[name]
        if self.lowp is not None:
            return self.lowp.data_ptr() + 2 * s.offset
        return self.params.data_ptr() + 4 * s.offset


def make_swaps(layout: Layout, params: torch.Tensor, names, device, out: Dict[str, int], lowp=None):
    """Descriptor array for vae_swap_axes over the named conv / convT weights (native
    [a][r][s][b] -> bf16 [b][r][s][a]) and the bf16 buffer holding the copies; `out` maps
    each name to its copy's device pointer.  lowp: the bf16 copy of `params` to read instead of
    the fp32 master (the same rounded values, half the bytes); it must be refreshed first."""
    specs = [layout.by_name[n] for n in names if n in layout.by_name]
    if len(specs) > L.SWAP_MAX:
        raise ValueError(f"{len(specs)} swapped weights > {L.SWAP_MAX} per vae_swap_axes launch")
    sizes = [(s.numel + 63) // 64 * 64 for s in specs]
    buf = torch.zeros(max(1, sum(sizes)), dtype=torch.bfloat16, device=device)
    descs = (L.SwapDesc * len(specs))()
    o = 0
    for i, (spec, n) in enumerate(zip(specs, sizes)):
        a, r, r2, b = spec.native_shape
        d = descs[i]
        if lowp is not None:
            d.src, d.src_dtype = lowp.data_ptr() + 2 * spec.offset, L.BF16
        else:
            d.src, d.src_dtype = params.data_ptr() + 4 * spec.offset, L.F32
        d.dst = buf.data_ptr() + 2 * o
        d.a, d.rs, d.b = a, r * r2, b
        out[spec.name] = d.dst
        o += n
    return descs, buf


class ZeroRegion:
    """Layout of a plan's zero region (the one fp32 buffer vae_step_begin clears): the pieces in the
    order they are added, each starting where the previous one's (padded) length ends."""

    def __init__(self):
        self.pieces = []         # (name, offset, numel)
        self.numel = 0

    def add(self, name: str, numel: int, pad: bool = True):
        """pad: round the piece's length up to 16 bytes, so the next piece starts aligned."""
        self.pieces.append((name, self.numel, numel))
        self.numel += _pad4(numel) if pad else numel

    def alloc(self, device) -> Dict[str, torch.Tensor]:
        """The zeroed buffer ("zero") and a view of it per piece."""
        zero = torch.zeros(self.numel, dtype=torch.float32, device=device)
        return {"zero": zero, **{name: zero[o:o + n] for name, o, n in self.pieces}}


class PlanBase:
    """What engine.TrainStep, dp and experiment.GraphedSteps rely on in a step plan.

    A plan has `net`, the buffers `x`, `recon`, `out`, `per_img`, `num_iter`, `step`, the zero
    region `zero` with `grads` and `metrics` in it, `loss_kind`, and the lists `fwd_calls` /
    `bwd_calls`.  What only some plans can do is declared here with a default that says no; a plan
    overrides what it supports."""

    side = None             # torch stream of the weight-gradient calls (run_calls); None: one stream
    side_all = True         # every SIDE_FNS call runs there (False: only the batches marked .side)
    wg_overlap = False      # the decoder's weight gradients as a side-stream batch (StepPlan)
    elbo_in_head = False    # the loss is evaluated by the head backward, not by the forward
    closer = None           # the loss that closes the forward in place of the ELBO (closers.py)
    term = None             # the loss's batch-coupled latent term (terms.py); answers the next two
    prior = None            # InfoVAE's prior sample (an input of the step)
    extra_term = None       # (name, one-element tensor): a fourth loss-dict entry (MMD, DIP_Loss)
    backward_done = False   # drop-in models: the backward of the last forward has run (models.py)
    deferred = False        # defer_reductions() has run: the backward leaves unreduced partials
    loss_names = ("loss", "Reconstruction_Loss", "KLD")     # the first three entries of `out`
    _loss_pending = False
    _bwd_raw = None         # set by a plan whose bwd_calls batches the calls it was built with

    def __init__(self, net):
        self.net = net
        self._keep = []            # ctypes structs referenced by the call lists
        self.fwd_calls: List = []
        self.bwd_calls: List = []

    # ------------------------------------------------------------------ optional capabilities
    @property
    def bwd_calls_raw(self):
        """The backward one call per op, before batching (what dp.plan_buckets cuts)."""
        return self.bwd_calls if self._bwd_raw is None else self._bwd_raw

    def batch_wgrads(self, ends):
        """Re-batch the weight gradients for backward segments ending at `ends` (indices into
        bwd_calls_raw); returns the ends in bwd_calls.  A plan that does not batch keeps both."""
        return ends

    def defer_reductions(self) -> bool:
        """Leave the backward's weight-gradient reductions to the optimizer launch; False: nothing is."""
        return False

    def use_device_eps(self, step: torch.Tensor, seed: int = 1265) -> bool:
        return False

    def use_device_prior(self, step: torch.Tensor, seed: int = 1265) -> bool:
        return False

    def draw_noise(self, eps: bool = True, prior: bool = True):
        """Fill the step's random inputs on the host side (a plan without any has nothing to do)."""

    # ------------------------------------------------------------------ shared helpers
    def g(self, name: str) -> int:
        s = self.net.layout.by_name[name]
        return self.grads.data_ptr() + 4 * s.offset

    def _add(self, lst, fn, arg):
        self._keep.append(arg)
        lst.append((fn, ctypes.byref(arg)))

    def size_workspaces(self):
        size_workspaces(self, [self.fwd_calls, self.bwd_calls])

    # ------------------------------------------------------------------ execution
    def _run(self, calls, stream):
        run_calls(self, calls, stream)

    def begin(self, stream=None):
        stream = stream if stream is not None else L.stream_ptr()
        L.call("vae_step_begin", self.zero.data_ptr(), self.zero.numel() * 4, self.step.data_ptr(), stream)

    def forward(self, stream=None):
        self._run(self.fwd_calls, stream if stream is not None else L.stream_ptr())
        self._loss_pending = self.elbo_in_head

    def backward(self, stream=None):
        if self.deferred:
            raise RuntimeError(DEFERRED_MSG)
        self._run(self.bwd_calls, stream if stream is not None else L.stream_ptr())
        self._loss_pending = False

    def loss_dict(self) -> Dict[str, float]:
        return dict(zip(self.loss_names, self.out.tolist()))


DEFERRED_MSG = ("this plan's backward is deferred to the optimizer launch of a TrainStep (defer_reductions): "
                "run on its own it leaves unreduced partial gradients.  Build a new plan for plan.backward(), "
                "for a step with a gradient exchange or for TrainStep(defer_reductions=False)")
