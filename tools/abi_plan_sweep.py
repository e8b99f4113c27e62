#!/usr/bin/env python3
"""What the library's host planning answers over a sweep of the conv / convT / linear / head C ABI (CPU only).

    python3 tools/abi_plan_sweep.py [--pkg DIR] [--out FILE] [--no-short]

A workspace query runs an entry point's whole planning with the launches switched off, so it needs no
device.  For every call of the sweep below the table has one line: the entry point, the settings, the
query's return code, the workspace bytes it reports and, for a failure, vae_last_error().  A refactor of
the native host side that must not change a plan is checked by running this on both checkouts (--pkg
points at the other one's pytorch-vae_amd, each with its own library) and comparing the files written
with --out; no digest is stored here.

Four parts:
  base      the six conv entries over dtype x batch x geometry x channels x wt_t x deterministic
  extended  fewer shapes, crossed with the transform kind of the gathered operand and of the
            epilogue (BatchNorm pointers set) and one of: residual, split_k = 4, the NCHW fp32
            image, dw_inner, a fused BatchNorm finalisation, a tensor that is not 16-byte aligned
  linear    the three linear entries over dtype x rows x (n, k) x mulv x deterministic
  head      the four decoder-head entries over dtype x batch x image size x channels x epilogue
            kind x deterministic (both of the head's routes, and the widths it rejects)
After each extended or linear query that reports a need, the entry itself is called with a workspace
one word short: planning must reject it.  Such a call may get as far as a launch (a staged weight
copy fits before the slab behind it is found short), and the tensors here are made-up addresses, so
these calls are made only where the process sees no GPU; elsewhere (and with --no-short) the lines
are left out.
"""
import argparse
import ctypes
import hashlib
import itertools
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FAKE = 1 << 24                      # aligned, never dereferenced (nothing launches)
GEOMS = [(4, 2, 3, 1), (16, 2, 3, 1), (32, 2, 3, 1), (16, 1, 3, 1), (16, 1, 1, 0), (32, 2, 4, 1)]   # h, stride, r, pad
CK = [(8, 32), (32, 64), (256, 512), (512, 256), (128, 128), (3, 32)]
CK_EXT = [(32, 64), (256, 512), (128, 128), (3, 32)]
NK = [(256, 2048), (2048, 512), (128, 128)]
CONV_FNS = ["vae_conv2d_fwd", "vae_conv2d_bwd_data", "vae_conv2d_bwd_filter",
            "vae_convT2d_fwd", "vae_convT2d_bwd_data", "vae_convT2d_bwd_filter"]
LINEAR_FNS = ["vae_linear_fwd", "vae_linear_bwd_data", "vae_linear_bwd_filter"]
HEAD_FNS = ["vae_head_fwd", "vae_head_bwd_data", "vae_head_bwd_filter", "vae_head_bwd"]
HEAD_C = [32, 64, 96, 128, 24, 40]       # (40: neither <= 32 nor a multiple of 32 — rejected)
VARIANTS = ["plain", "residual", "split4", "residual+split4", "nchw", "dw_inner", "finalize", "odd_aux"]


def _xform(L, kind, channels):
    x = L.Xform(kind=kind, channels=channels, slope=0.01, count=64.0, eps=1e-5, momentum=0.1)
    for f in ("sum", "sumsq", "gamma", "beta", "dgamma", "dbeta", "aux"):
        setattr(x, f, FAKE)
    return x


def conv_args(L, fn, dtype, n, geom, ck, wt_t, det):
    h, stride, r, pad = geom
    c, k = ck
    p = h * stride if "convT" in fn else h // stride         # (ConvTranspose2d doubles, Conv2d halves)
    a = L.ConvArgs(dtype=dtype, n=n, h=h, w=h, c=c, k=k, p=p, q=p, r=r, stride=stride, pad=pad, deterministic=det)
    for f in ("x", "wt", "y", "dy", "dx", "dw"):
        setattr(a, f, FAKE)
    if wt_t:
        a.wt_t = FAKE
    a.x_xf = L.Xform(kind=L.X_NONE, channels=c)
    a.dy_xf = L.Xform(kind=L.X_NONE, channels=k)
    a.dx_epi = L.Xform(kind=L.X_NONE, channels=c)
    return a


def extend(L, a, kind_g, kind_e, variant):
    """The BatchNorm pointers, the two transform kinds and one variant on top of conv_args.  Returns
    what must stay alive as long as `a` is used."""
    keep = None
    a.x_xf, a.dy_xf, a.dx_epi = _xform(L, kind_g, a.c), _xform(L, kind_g, a.k), _xform(L, kind_e, a.c)
    for f in ("bias", "y_sum", "y_sumsq", "dx_dgamma", "dx_dbeta", "db"):
        setattr(a, f, FAKE)
    if "residual" in variant:
        a.residual = FAKE
        a.residual_xf = L.Xform(kind=L.X_ACT, channels=a.k, slope=0.01)
    if "split4" in variant:
        a.split_k = 4
    if variant == "nchw":
        a.x_nchw_f32 = 1
    if variant == "dw_inner":
        a.dw_inner = 8
    if variant == "finalize":
        keep = L.BnArgs(mode=0, xf=_xform(L, L.X_BN_ACT, a.k), table=FAKE)
        a.bn_finalize = ctypes.pointer(keep)
    if variant == "odd_aux":
        a.dx_epi.aux = FAKE + 2
        a.dy_xf.aux = FAKE + 2
    return keep


def linear_args(L, dtype, m, nk, mulv, det, kind):
    n, k = nk
    a = L.LinearArgs(dtype=dtype, m=m, n=n, k=k, samples=1, deterministic=det)
    for f in ("x", "wt", "bias", "y", "dy", "dx", "dw", "db", "dx_dgamma", "dx_dbeta"):
        setattr(a, f, FAKE)
    a.x_xf, a.dx_epi = _xform(L, kind, k), _xform(L, kind, k)
    if mulv:
        a.mulv = a.eps = a.dmulv = FAKE
        a.dy_f32 = 1
    return a


def head_args(L, dtype, n, hw, c, kind, det):
    a = L.HeadArgs(dtype=dtype, n=n, h=hw, w=hw, c=c, samples=1, deterministic=det)
    for f in ("x", "wt", "bias", "target", "recon", "sse", "coef", "dx", "dx_dgamma", "dx_dbeta", "dw", "db"):
        setattr(a, f, FAKE)
    a.x_xf, a.dx_epi = _xform(L, L.X_BN_ACT, c), _xform(L, kind, c)
    return a


def query(L, fn, a):
    """(return code, workspace bytes, error text) of fn's workspace query for `a`."""
    lib = L.load()
    q, op = L.WS_QUERY[fn]
    out = ctypes.c_size_t(0)
    rc = getattr(lib, q)(ctypes.byref(a), op, ctypes.byref(out))
    return rc, int(out.value), (lib.vae_last_error().decode(errors="replace") if rc else "")


def short_call(L, fn, a, need):
    """(return code, error text) of the entry itself with a workspace one word short of `need`."""
    lib = L.load()
    a.workspace, a.workspace_bytes = FAKE, need - 4
    rc = getattr(lib, fn)(ctypes.byref(a), None)
    return rc, (lib.vae_last_error().decode(errors="replace") if rc else "")


def no_gpu():
    import torch
    return not torch.cuda.is_available()


def table(L, ck=CK, ck_ext=CK_EXT, nk=NK, short=True):
    """The sweep's lines, in a fixed order."""
    short = short and no_gpu()
    rows = []

    def line(part, fn, key, a):
        rc, need, err = query(L, fn, a)
        rows.append(f"{part} {fn} {key} rc={rc} need={need} {err}".rstrip())
        if short and part != "base" and rc == 0 and need > 0:
            src, serr = short_call(L, fn, a, need)
            rows.append(f"{part} {fn} {key} short rc={src} {serr}".rstrip())

    for fn in CONV_FNS:
        for dtype, n, geom, s, wt_t, det in itertools.product((L.BF16, L.F32), (1, 7, 64), GEOMS, ck, (1, 0), (0, 1)):
            line("base", fn, f"dt={dtype} n={n} geom={geom} ck={s} wt_t={wt_t} det={det}",
                 conv_args(L, fn, dtype, n, geom, s, wt_t, det))
    kinds = (L.X_NONE, L.X_ACT, L.X_BN_ACT, L.X_BN_DY)
    for fn in CONV_FNS:
        for dtype, n, geom, s, wt_t, kg, ke, v in itertools.product((L.BF16, L.F32), (7, 64), GEOMS, ck_ext, (1, 0),
                                                                    kinds, kinds, VARIANTS):
            a = conv_args(L, fn, dtype, n, geom, s, wt_t, 0)
            keep = extend(L, a, kg, ke, v)
            line("ext", fn, f"dt={dtype} n={n} geom={geom} ck={s} wt_t={wt_t} g={kg} e={ke} {v}", a)
            del keep
    for fn in LINEAR_FNS:
        for dtype, m, s, mulv, det, kind in itertools.product((L.BF16, L.F32), (1, 7, 64, 320), nk, (1, 0), (0, 1),
                                                              (L.X_NONE, L.X_BN_ACT)):
            line("linear", fn, f"dt={dtype} m={m} nk={s} mulv={mulv} det={det} xf={kind}",
                 linear_args(L, dtype, m, s, mulv, det, kind))
    for fn in HEAD_FNS:
        for dtype, n, hw, c, kind, det in itertools.product((L.BF16, L.F32), (2, 64), (64, 32), HEAD_C,
                                                            (L.X_NONE, L.X_ACT, L.X_BN_ACT), (0, 1)):
            line("head", fn, f"dt={dtype} n={n} hw={hw} c={c} e={kind} det={det}", head_args(L, dtype, n, hw, c, kind, det))
    return rows


def digest(rows) -> str:
    return hashlib.sha256("\n".join(rows).encode()).hexdigest()[:16]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pkg", default=os.path.join(REPO, "pytorch-vae_amd"),
                    help="the pytorch-vae_amd directory to sweep (default: this checkout's)")
    ap.add_argument("--out", default="", help="file for the table, one line per call")
    ap.add_argument("--no-short", action="store_true", help="leave out the calls with a short workspace")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.pkg))
    from vae_amd import _lib as L
    rows = table(L, short=not args.no_short)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(rows) + "\n")
    failed = sum(" rc=0" not in r for r in rows)
    print(f"{len(rows)} lines ({failed} with an error)  {digest(rows)}")


if __name__ == "__main__":
    main()
