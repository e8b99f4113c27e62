"""Call lists: what a step plan is made of, and the functions that size, batch and launch them.

A plan (net.StepPlan, vq.VQStepPlan) is two lists of (entry point, argument) pairs.  The argument of
an entry has one of four shapes:
  * ctypes.byref(struct)              — most calls (`plan._add`);
  * a tuple of scalars                — the scalar-argument entry points (vae_pad_channels, ...);
  * a tuple of byrefs                 — vae_convT2d_fwd_recon (ConvArgs, ReconArgs);
  * an L.FilterBatch                  — vae_conv_bwd_filter_batch over several weight-gradient calls.
`call_one` launches an entry; `structs` gives the argument structs behind it, whatever its shape.
What a plan itself must offer is plan.PlanBase.
"""
from __future__ import annotations

import ctypes
from typing import List

import torch

from . import _lib as L

BATCH_FN = "vae_conv_bwd_filter_batch"
DEFERRED_FNS = frozenset(("vae_conv2d_bwd_filter", "vae_convT2d_bwd_filter", "vae_unpad_accumulate"))
SIDE_FNS = frozenset(("vae_conv2d_bwd_filter", "vae_convT2d_bwd_filter", "vae_linear_bwd_filter",
                      "vae_unpad_accumulate"))     # (follows its padded weight gradient)
_BYREF = type(ctypes.byref(ctypes.c_int32()))


def structs(ref) -> List[ctypes.Structure]:
    """The argument structs behind one call-list entry ([] for None or a scalar tuple)."""
    if isinstance(ref, L.FilterBatch):
        return ref.args
    if isinstance(ref, _BYREF):
        return [ref._obj]
    if isinstance(ref, tuple):
        return [r._obj for r in ref if isinstance(r, _BYREF)]
    return []


def on_side(plan, fn, ref) -> bool:
    """Whether an entry is a weight-gradient call that runs on the plan's side stream (when it has
    one): a batch marked for it, or with `side_all` every weight-gradient call."""
    if fn == BATCH_FN:
        return ref.side
    return plan.side_all and fn in SIDE_FNS


def batch_filter_calls(calls, ends, splits=(), enabled: bool = True):
    """Weight gradients are read only by the optimizer, so within a backward segment they can
    run after the segment's data-gradient chain and together: the conv / convT bwd_filter calls
    of each segment become one vae_conv_bwd_filter_batch call (grouped launches) at its end,
    followed by the calls that must follow them (vae_unpad_accumulate reads the padded first-layer
    weight gradient).  `splits`: raw call indices inside a segment where the weight gradients so
    far are emitted as a batch of their own that runs on the plan's side stream (run_calls).
    enabled=False: one call per layer, as built.  Returns (new call list, new segment ends)."""
    if not enabled:
        return list(calls), list(ends)
    out, new_ends, lo = [], [], 0

    def emit(deferred, side):
        wg = [(fn, ref) for fn, ref in deferred if fn != "vae_unpad_accumulate"]
        if len(wg) > 1 or (side and wg):
            b = L.FilterBatch(wg)
            b.side = side
            out.append((BATCH_FN, b))
            unpads = [(fn, ref) for fn, ref in deferred if fn == "vae_unpad_accumulate"]
            if side:
                # they read the batch's padded gradients: same (side) stream, right behind it
                b.after = unpads
            else:
                out.extend(unpads)
        else:
            out.extend(deferred)

    for end in ends:
        deferred = []
        for i in range(lo, end):
            if i in splits and deferred:
                emit(deferred, True)
                deferred = []
            fn, ref = calls[i]
            if fn in DEFERRED_FNS:
                deferred.append((fn, ref))
            else:
                out.append((fn, ref))
        emit(deferred, False)
        new_ends.append(len(out))
        lo = end
    return out, new_ends


def size_workspaces(plan, call_lists):
    """Give a plan's calls their workspace: each call's need is queried from the library
    (vaehip.h vae_*_workspace_size, which runs the call's own planning without launching), and
    the calls of the main chain share one buffer sized to the largest need, the weight-gradient
    calls of the side stream (run_calls) another — the two chains run concurrently.  A call
    whose need is 0 gets no workspace (the same plan).  Sets plan.workspace / plan.workspace_side
    and plan.workspace_need = {chain: bytes}."""
    dev = plan.net.device
    need = {"main": 0, "side": 0}
    sized = []
    for calls in call_lists:
        for fn, ref in calls:
            if fn == BATCH_FN:
                arg = ref
                b = ref.workspace_size()
            elif fn not in L.WS_QUERY:
                continue
            else:
                arg = ref._obj
                b = L.workspace_size(fn, arg)
            deferred = any(getattr(a, "defer_reduce", 0) for a in structs(ref))
            chain = "side" if plan.side is not None and on_side(plan, fn, ref) else "main"
            if deferred and b > 0:
                # partial rows read later by the optimizer (vae_adam_step_ex): a buffer of its own
                chain = f"deferred{len(need)}"
                need[chain] = 0
            need[chain] = max(need[chain], b)
            sized.append((arg, b, chain))
    bufs = {c: torch.empty(max(1, (n + 3) // 4), dtype=torch.float32, device=dev) for c, n in need.items()}
    for arg, b, chain in sized:
        if b > 0:
            arg.workspace = bufs[chain].data_ptr()
            arg.workspace_bytes = bufs[chain].numel() * 4
        else:
            arg.workspace, arg.workspace_bytes = None, 0
    plan.workspace, plan.workspace_side, plan.workspace_need = bufs["main"], bufs["side"], need
    plan.workspace_deferred = [v for k, v in bufs.items() if k.startswith("deferred")]


def run_calls(plan, calls, stream):
    """Launch a call list on `stream`.  When the plan has a side stream (`plan.side`, and
    `stream` is the current torch stream), every weight-gradient call waits for the work queued
    on `stream` before it and runs on the side stream; the side stream is joined back into
    `stream` at the end of the list.  Recorded inside a HIP graph capture this becomes the
    graph's fork/join edges, so the replayed graph runs the two chains concurrently."""
    if plan.net.swaps_stale:
        # the swapped-axes weight copies trail the last optimizer step (a TrainStep refreshes them
        # inside its next step's head launch): bring them up to date before anything reads them
        plan.net.refresh_swaps(stream)
    side = plan.side
    main = torch.cuda.current_stream() if side is not None else None
    if main is not None and main.cuda_stream != stream:
        side = None                          # an explicit foreign stream: keep everything on it
    forked = False
    for fn, arg in calls:
        if side is not None and on_side(plan, fn, arg):
            side.wait_stream(main)
            call_one(fn, arg, side.cuda_stream)
            forked = True
        else:
            call_one(fn, arg, stream)
    if forked:
        main.wait_stream(side)


def call_one(fn, arg, stream):
    """One entry of a plan's call list (struct argument, scalar-argument tuple or a batch of
    weight-gradient calls) on `stream`."""
    if fn == BATCH_FN:
        arg(stream)
    elif isinstance(arg, tuple):
        L.call(fn, *arg, stream)
    else:
        L.call(fn, arg, stream)
