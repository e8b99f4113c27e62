#!/usr/bin/env python3
"""Run one training step call by call with a device sync after each, printing every call first
(diagnostic: names the launch that faults or fails).  python3 tools/debug_calls.py [vq|vanilla] [B]"""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "pytorch-vae_amd")]
import torch  # noqa: E402


def main():
    arch = sys.argv[1] if len(sys.argv) > 1 else "vq"
    B = int(sys.argv[2]) if len(sys.argv) > 2 else 4
    from vae_amd import _lib as L
    from vae_amd.calls import call_one, structs
    torch.cuda.set_device(0)
    if arch == "vq":
        from vae_amd.vq import VQNet, VQStepPlan
        net = VQNet(dtype=torch.bfloat16, device="cuda", generator=torch.Generator().manual_seed(0))
        plan = VQStepPlan(net, B)
    else:
        from vae_amd.net import StepPlan, VAENet
        net = VAENet(latent_dim=128, dtype=torch.bfloat16, device="cuda", generator=torch.Generator().manual_seed(0))
        plan = StepPlan(net, B)
    plan.x.copy_(torch.rand(plan.x.shape, device="cuda"))
    torch.cuda.synchronize()
    st = L.stream_ptr()
    print("swaps", sum(len(d) for d in net.swap_descs), flush=True)
    for i, (fn, ref) in enumerate(plan.fwd_calls + plan.bwd_calls):
        desc = ""
        for a in (a for a in structs(ref) if isinstance(a, L.ConvArgs)):
            desc += f" n={a.n} h={a.h} c={a.c} k={a.k} r={a.r} s={a.stride} wt_t={bool(a.wt_t)} ws={a.workspace_bytes}"
        print(f"{i:3d} {fn}{desc}", flush=True)
        call_one(fn, ref, st)
        torch.cuda.synchronize()
    print("ok", flush=True)


if __name__ == "__main__":
    main()
