#!/usr/bin/env python3
"""Position-independent digest of everything a plan's launches are made from (diagnostic, CPU only).

    python3 tools/plan_fingerprint.py [--pkg DIR] [--only NAME,..] [--dump DIR]

For each configuration below: the forward / backward call lists (as built and batched), the
vae_step_begin_ex arguments, the gradient buckets of a two-bucket exchange and the lists re-batched
for them, the lists again after defer_reductions(), and the size of the zero region.  Every argument
struct is written out field by field; an integer that points into a tensor reachable from the plan or
its net becomes (allocation in order of first appearance, byte offset), one that is the address of an
argument struct becomes that struct, so two builds of the same plan give the same digest wherever
their buffers land.  A host-side refactor that must not change a launch is checked by running this on
both checkouts (--pkg points at the other one's pytorch-vae_amd) and comparing the tables;
--dump writes the JSON behind each digest for diffing.

Nothing is launched: plans build on device="cpu" with the two launches of construction
(vae_cast_bf16, vae_swap_axes) stubbed; the workspace queries run the library's planning, which needs
no device.  The call-list entries are read by their shape (byref / tuples / FilterBatch) rather than
through vae_amd.calls so that the same file reads a checkout from before that module existed.
"""
import argparse
import bisect
import contextlib
import ctypes
import hashlib
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

AE_BIG = [128, 256, 512, 1024, 2048]
WIDE = [64, 64, 128, 256, 512]          # with head_kernels=False: the head on the conv-GEMM route
CENTER = {"kind": "center", "mask": torch.ones(64, 64)}
# name -> (net kind, net arguments, batch, plan arguments); bf16 unless "fp32" is in the name
CONFIGS = {
    "vanilla_b64": ("vae", {}, 64, {}),
    "betaH_b32": ("vae", {}, 32, dict(loss="betaH", kld_weight=2.5e-4)),
    "iwae_b64_s5": ("vae", {}, 64, dict(loss="iwae", kld_weight=2.5e-4, samples=5)),
    "info_b16": ("vae", {}, 16, dict(loss="info")),
    "ae_big_b8": ("vae", dict(hidden_dims=AE_BIG), 8, dict(kld_weight=0.0)),
    "per_op_b16": ("vae", {}, 16, dict(latent_kernels=False, pad_rgb=False)),
    "unbatched_b16": ("vae", {}, 16, dict(batch_wgrads=False)),
    "gemm_head_b4": ("vae", dict(hidden_dims=WIDE), 4, dict(head_kernels=False)),
    "fuse_bn_b4": ("vae", {}, 4, dict(fuse_bn=True, bn_in_consumer=False)),
    "dropin_train_b4": ("vae", {}, 4, dict(fused_loss=False)),
    "dropin_eval_b4": ("vae", {}, 4, dict(fused_loss=False, training=False)),
    "vanilla_fp32_b4": ("vae", {}, 4, {}),
    "vq_b8": ("vq", {}, 8, {}),
    "vq_fp32_b8": ("vq", {}, 8, {}),
    # the losses with a batch-coupled latent term (vae_amd/terms.py) and their neighbours
    "dip_b16": ("vae", {}, 16, dict(loss="dip")),
    "miwae_b4_m2k3": ("vae", {}, 4, dict(loss="miwae", samples=3, estimates=2)),
    "betaB_b16": ("vae", {}, 16, dict(loss="betaB")),
    "info_dropin_b4": ("vae", {}, 4, dict(loss="info", fused_loss=False)),
    "dip_dropin_b4": ("vae", {}, 4, dict(loss="dip", fused_loss=False)),
    "miwae_dropin_b2": ("vae", {}, 2, dict(loss="miwae", fused_loss=False, samples=2, estimates=2)),
    "info_per_op_b16": ("vae", {}, 16, dict(loss="info", latent_kernels=False)),
    "dip_fp32_b4": ("vae", {}, 4, dict(loss="dip")),
    "center_b4": ("vae", {}, 4, dict(recon_loss=CENTER, kld_weight=0.0)),
    # the losses that close the forward themselves (vae_amd/closers.py), with their drop-in and eval
    # plans, which have no loss call, and the wide head under a closer
    "logcosh_b16": ("vae", {}, 16, dict(loss="logcosh", alpha=10.0, beta=2.0, kld_weight=2.5e-4)),
    "logcosh_per_op_b4": ("vae", {}, 4, dict(loss="logcosh", alpha=10.0, latent_kernels=False, pad_rgb=False)),
    "logcosh_fp32_b4": ("vae", {}, 4, dict(loss="logcosh", alpha=10.0)),
    "logcosh_dropin_b4": ("vae", {}, 4, dict(loss="logcosh", alpha=10.0, fused_loss=False)),
    "logcosh_eval_b4": ("vae", {}, 4, dict(loss="logcosh", alpha=10.0, training=False)),
    "logcosh_wide_b4": ("vae", dict(hidden_dims=WIDE), 4, dict(loss="logcosh", alpha=10.0, head_kernels=False)),
    "mssim_b4": ("vae", {}, 4, dict(recon_loss={"kind": "mssim", "window": [1 / 11] * 11}, kld_weight=0.0)),
    "center_wide_b4": ("vae", dict(hidden_dims=WIDE), 4, dict(recon_loss=CENTER, kld_weight=0.0, head_kernels=False)),
    "center_eval_b4": ("vae", {}, 4, dict(recon_loss=CENTER, kld_weight=0.0, training=False, fused_loss=False)),
}


@contextlib.contextmanager
def no_launches(L):
    """Let only the workspace queries through to the library; the current stream is 0."""
    call, stream_ptr = L.call, L.stream_ptr

    def query_only(name, *args):
        if name.endswith("workspace_size"):
            call(name, *args)

    L.call, L.stream_ptr = query_only, lambda: 0
    try:
        yield
    finally:
        L.call, L.stream_ptr = call, stream_ptr


def build(name, **override):
    """(net, plan) of a configuration on the CPU; `override` replaces plan arguments."""
    from vae_amd import _lib as L
    kind, net_kw, batch, plan_kw = CONFIGS[name]
    dtype = torch.float32 if "fp32" in name else torch.bfloat16
    gen = torch.Generator().manual_seed(0)
    with no_launches(L):
        if kind == "vq":
            from vae_amd.vq import VQNet, VQStepPlan
            net = VQNet(dtype=dtype, device="cpu", generator=gen, **net_kw)
            plan = VQStepPlan(net, batch, **{**plan_kw, **override})
        else:
            from vae_amd.net import StepPlan, VAENet
            net = VAENet(latent_dim=128, dtype=dtype, device="cpu", generator=gen, **net_kw)
            plan = StepPlan(net, batch, **{**plan_kw, **override})
    return net, plan


class Writer:
    """Serialises call lists and structs with pointers replaced by what they point at."""

    def __init__(self, *roots):
        import torch
        self.torch = torch
        self.roots = roots           # (spans: storage start -> end; structs: address -> ctypes struct)
        self.rescan()

    def rescan(self):
        """Start a stage: what is reachable now, numbered afresh (batch_wgrads / defer_reductions
        re-size the workspaces, and a new buffer may land where a freed one was)."""
        self.spans, self.structs, self.buf_ids, self.struct_ids = {}, {}, {}, {}
        seen = set()
        for r in self.roots:
            self._scan(r, seen, 0)
        self.starts = sorted(self.spans)

    def _scan(self, o, seen, depth):
        if id(o) in seen or depth > 10:
            return
        seen.add(id(o))
        if isinstance(o, self.torch.Tensor):
            st = o.untyped_storage()
            if st.nbytes():
                self.spans[st.data_ptr()] = st.data_ptr() + st.nbytes()
        elif isinstance(o, ctypes.Structure):
            self.structs[ctypes.addressof(o)] = o
        elif isinstance(o, dict):
            for v in o.values():
                self._scan(v, seen, depth + 1)
        elif isinstance(o, (list, tuple)):
            for v in o:
                self._scan(v, seen, depth + 1)
        elif hasattr(o, "_obj"):                              # byref(struct)
            self._scan(o._obj, seen, depth + 1)
        elif type(o).__module__.startswith("vae_amd") and hasattr(o, "__dict__"):
            for v in vars(o).values():
                self._scan(v, seen, depth + 1)

    def integer(self, v):
        if v in self.structs:
            first = v not in self.struct_ids
            k = self.struct_ids.setdefault(v, len(self.struct_ids))
            return ["struct", k, self.value(self.structs[v])] if first else ["struct", k]
        i = bisect.bisect_right(self.starts, v) - 1
        if i >= 0 and v < self.spans[self.starts[i]]:
            base = self.starts[i]
            return ["buf", self.buf_ids.setdefault(base, len(self.buf_ids)), v - base]
        return v

    def value(self, v):
        if v is None or isinstance(v, (str, bool)):
            return v
        if isinstance(v, int):
            return self.integer(v)
        if isinstance(v, float):
            return repr(v)
        if isinstance(v, ctypes.Structure):
            self.struct_ids.setdefault(ctypes.addressof(v), len(self.struct_ids))
            return [type(v).__name__] + [[f[0], self.value(getattr(v, f[0]))] for f in v._fields_]
        if isinstance(v, ctypes.Array):
            return [self.value(x) for x in v]
        if isinstance(v, ctypes._Pointer):
            return ["ptr", self.value(v.contents)] if v else None
        if isinstance(v, (list, tuple)):
            return [self.value(x) for x in v]
        raise TypeError(f"plan_fingerprint: {type(v)}")

    def entry(self, fn, ref):
        if ref is None:
            return [fn, None]
        if hasattr(ref, "calls"):                             # FilterBatch
            return [fn, "batch", bool(ref.side), self.calls(ref.calls), self.calls(ref.after),
                    self.value(ref.workspace), ref.workspace_bytes]
        if isinstance(ref, tuple) and ref and hasattr(ref[0], "_obj"):
            return [fn, "refs"] + [self.value(r._obj) for r in ref]
        if isinstance(ref, tuple):
            return [fn, "scalars", self.value(ref)]
        return [fn, "ref", self.value(ref._obj)]

    def calls(self, lst):
        return [self.entry(fn, ref) for fn, ref in lst]


def describe(name, **override):
    """The JSON-able description of one configuration (see the module docstring)."""
    from vae_amd import dp
    from vae_amd.engine import begin_args
    net, plan = build(name, **override)
    step = torch.zeros(1, dtype=torch.int32)
    w = Writer(plan, net, step)
    out = {"zero": plan.zero.numel()}

    def lists(tag):
        w.rescan()
        for k in ("fwd_calls", "bwd_calls", "bwd_calls_raw"):
            out[f"{tag}.{k}"] = w.calls(getattr(plan, k, plan.bwd_calls))
        out[f"{tag}.workspace_need"] = sorted(plan.workspace_need.items())

    lists("built")
    args, k = begin_args(plan, step)
    out["begin"] = [w.value(args), k]
    from vae_amd import _lib as L
    with no_launches(L):
        raw = getattr(plan, "bwd_calls_raw", plan.bwd_calls)
        buckets = dp.plan_buckets(raw, plan.grads, net.layout, 2)
        ends = [b[0] for b in buckets]
        if hasattr(plan, "batch_wgrads"):
            ends = plan.batch_wgrads(ends)
        out["buckets"] = [list(b) for b in buckets]
        out["ends"] = list(ends)
        lists("bucketed")
        out["deferred"] = bool(plan.defer_reductions()) if hasattr(plan, "defer_reductions") else False
        lists("deferred")
    return out


def digest(desc) -> str:
    return hashlib.sha256(json.dumps(desc, sort_keys=True).encode()).hexdigest()[:16]


def fingerprint(name, **override) -> str:
    return digest(describe(name, **override))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pkg", default=os.path.join(REPO, "pytorch-vae_amd"),
                    help="the pytorch-vae_amd directory to fingerprint (default: this checkout's)")
    ap.add_argument("--only", default="", help="comma list of configuration names")
    ap.add_argument("--dump", default="", help="directory for one JSON file per configuration")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.pkg))
    if args.dump:
        os.makedirs(args.dump, exist_ok=True)
    for name in [n for n in args.only.split(",") if n] or list(CONFIGS):
        desc = describe(name)
        if args.dump:
            with open(os.path.join(args.dump, name + ".json"), "w") as f:
                json.dump(desc, f, indent=1, sort_keys=True)
        print(f"{name:18s} {digest(desc)}  fwd {len(desc['built.fwd_calls']):3d}  bwd {len(desc['built.bwd_calls']):3d}"
              f"  zero {desc['zero']}", flush=True)


if __name__ == "__main__":
    main()
