"""Every BatchNorm coefficient builder that has an entry point of its own, against fp64 BatchNorm.

The library turns a producer's replicated sums into a per-channel table (vaehip.h vae_xform.table):
vae_bn_finalize (modes 0, 1, 2), the tables vae_bn_apply builds itself from the statistics
(vae_igemm.hpp tab_fill: the one-round fast path and the plain loop) or copies from a finalised table,
and the finalisation a producing conv call carries (vae_conv_args.bn_finalize).  The reference is
tests/bn_ref.py in fp64 from the very fp32 replicas the kernel reads (real small tensors y, g by the
recipe there; tests/test_bn_ref.py pins it against torch and shows fp32 reaches 1e-6).

Bars: fp32 table rows, running statistics, dgamma_out / dbeta_out: 1e-5 of the row's max-abs
(test_gpu_cgemm.check_wgrad's bar for fp32 BatchNorm affine gradients).  The closed-form bias
gradient db, analytically zero: |got - start| <= 1e-6 · (|A·Σg| + |B·Σy| + |C·M|) per channel, with
each term alone at least 100 bars on at least 98 % of the channels (bn_ref.db_terms_visible).
bf16 outputs of vae_bn_apply: within 2^-8 · |ref| of the reference elementwise (+ 1e-6 · (|A g| + |B y| +
|C|) for BN_DY), see check_out.  Every measured error is printed."""
import ctypes
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

import bn_ref as R
from gpu_util import give_workspace, launched, nhwc, rel, to_nchw, tol

pytestmark = pytest.mark.gpu

ROW_BAR, DB_BAR, GUARD = 1e-5, 1e-6, 64
NAN = float("nan")


def _L():
    from vae_amd import _lib as L
    return L


def _stream():
    return torch.cuda.current_stream().cuda_stream


def guarded(values):
    """(device buffer of `values` followed by GUARD NaN floats, the view of the values)."""
    buf = torch.full((values.numel() + GUARD,), NAN, device="cuda")
    buf[:values.numel()] = values.flatten().float().cuda()
    return buf, buf[:values.numel()]


def guard_intact(buf, n):
    return bool(torch.isnan(buf[n:]).all())


class Dev:
    """A bn_ref case on the device: the replicated statistics (NaN pads kept) and the parameters."""

    def __init__(self, c):
        self.c = c
        self.t = {k: v.contiguous().cuda() for k, v in c.bufs.items()}
        self.t["gamma"], self.t["beta"] = c.gamma.cuda(), c.beta.cuda()
        if c.shift is not None:
            self.t["shift"] = c.shift.cuda()

    def xf(self, kind=0, count=None):
        L, c = _L(), self.c
        x = L.Xform(kind=kind, channels=c.C, slope=R.SLOPE, count=float(c.M if count is None else count), eps=R.EPS,
                    momentum=R.MOMENTUM)
        for k in ("sum", "sumsq", "dgamma", "dbeta", "gamma", "beta", "shift"):
            if k in self.t:
                setattr(x, k, self.t[k].data_ptr())
        x.reps, x.rstride = c.R, c.rstride
        return x


def finalize(x, mode, table, db=None):
    L = _L()
    a = L.BnArgs(mode=mode)
    a.xf, a.table = x, table.data_ptr()
    if db is not None:
        a.db = db.data_ptr()
    L.call("vae_bn_finalize", ctypes.byref(a), _stream())
    torch.cuda.synchronize()


def check_rows(tag, table, C, ref, names):
    tab = table[:len(names) * C].cpu().view(len(names), C)
    errs = {k: R.row_err(tab[i], getattr(ref, k)) for i, k in enumerate(names)}
    print(f"{tag}: " + ", ".join(f"{k} {e:.2e}" for k, e in errs.items()) + f" (bar {ROW_BAR})")
    for k, e in errs.items():
        assert e < ROW_BAR, (tag, k, e)
    return tab


# C, reps, pad floats between the replicas (rstride = C + pad; reps = 1: rstride = 0), M
GRID = [(3, 1, 0, 192), (24, 5, 8, 192), (64, 8, 0, 192), (64, 2, 8, 192), (96, 2, 0, 32), (130, 9, 8, 64),
        (512, 32, 0, 20), (1000, 32, 8, 8), (4096, 1, 0, 8), (4096, 5, 8, 8)]


def grid_case(C, reps, pad, M, centred):
    return R.make_case(C, reps, M, rstride=C + pad, centred=centred)


def random_running(C, seed):
    gen = torch.Generator().manual_seed(seed)
    return torch.randn(C, generator=gen), 0.5 + torch.rand(C, generator=gen)


# ------------------------------------------------------------------------------------- (a) mode 0
@pytest.mark.parametrize("centred", [False, True], ids=["shift", "noshift"])
@pytest.mark.parametrize("C,reps,pad,M", GRID)
def test_finalize_forward(C, reps, pad, M, centred):
    """Mode 0: the [4][C] forward table and the running statistics from random start values; the table
    is the same bit for bit with and without running pointers; NaN pads between the replicas and the
    NaN guard floats behind every output stay where they are."""
    c = grid_case(C, reps, pad, M, centred)
    d = Dev(c)
    tag = f"fwd C={C} R={reps} rstride={c.rstride} M={M} {'no shift' if centred else 'shift'}"
    t1 = torch.full((4 * C + GUARD,), NAN, device="cuda")
    log = launched(lambda: finalize(d.xf(), 0, t1))
    assert "bn_finalize_kernel" in log, log
    check_rows(tag, t1, C, c.ref, R.FWD_ROWS)
    assert guard_intact(t1, 4 * C)
    rm0, rv0 = random_running(C, C + reps)
    (rmb, rm), (rvb, rv) = guarded(rm0), guarded(rv0)
    x = d.xf()
    x.running_mean, x.running_var = rm.data_ptr(), rv.data_ptr()
    t2 = torch.full((4 * C + GUARD,), NAN, device="cuda")
    finalize(x, 0, t2)
    assert torch.equal(t1[:4 * C], t2[:4 * C]) and guard_intact(t2, 4 * C)
    want_m, want_v = R.running_update(rm0, rv0, c.ref)
    e_m, e_v = R.row_err(rm.cpu(), want_m), R.row_err(rv.cpu(), want_v)
    print(f"{tag}: running mean {e_m:.2e}, running var {e_v:.2e} (bar {ROW_BAR})")
    assert e_m < ROW_BAR and e_v < ROW_BAR
    assert guard_intact(rmb, C) and guard_intact(rvb, C)
    for k in ("sum", "sumsq"):                      # the statistics are read-only
        assert torch.equal(d.t[k].cpu().nan_to_num(nan=7.0), c.bufs[k].nan_to_num(nan=7.0))


def crafted(sum_, sumsq, M, reps, gamma=None, seed=0):
    """A statistics set given as [C] totals (no tensors behind it), split like the others."""
    gen = torch.Generator().manual_seed(seed)
    C = sum_.numel()
    gamma = (0.8 + 0.4 * torch.rand(C, generator=gen)) if gamma is None else gamma
    beta = (torch.rand(C, generator=gen) * 2 - 1) * 0.1
    bufs = {"sum": R.split_replicas(sum_, reps, C + 8, gen), "sumsq": R.split_replicas(sumsq, reps, C + 8, gen)}
    rows = {k: R.replica_rows(v, C) for k, v in bufs.items()}
    ref = R.bn_tables(rows["sum"], rows["sumsq"], None, None, None, gamma, beta, M)
    return SimpleNamespace(C=C, R=reps, M=M, rstride=C + 8 if reps > 1 else 0, gamma=gamma, beta=beta, shift=None,
                           bufs=bufs, rows=rows, ref=ref)


@pytest.mark.parametrize("reps", [1, 5])
def test_finalize_forward_count_one(reps):
    """count = 1 takes the unb = var branch: no division by zero, every row finite, the running
    variance moves by momentum · var.  The statistics are crafted (Σd² = (Σd)² + v, v in [0.5, 2]) so
    that the variance the branch must keep is not zero."""
    gen = torch.Generator().manual_seed(11)
    C = 70
    s = torch.randint(-32, 33, (C,), generator=gen).double() / 16
    v = 0.5 + 1.5 * torch.rand(C, generator=gen, dtype=torch.float64)
    c = crafted(s, s * s + v, 1, reps)
    d = Dev(c)
    rm0, rv0 = random_running(C, 5)
    (rmb, rm), (rvb, rv) = guarded(rm0), guarded(rv0)
    x = d.xf()
    x.running_mean, x.running_var = rm.data_ptr(), rv.data_ptr()
    t = torch.full((4 * C + GUARD,), NAN, device="cuda")
    finalize(x, 0, t)
    tab = check_rows(f"fwd count=1 R={reps}", t, C, c.ref, R.FWD_ROWS)
    assert torch.isfinite(tab).all() and torch.isfinite(rm).all() and torch.isfinite(rv).all()
    assert torch.equal(c.ref.unb, c.ref.var)
    want_m, want_v = R.running_update(rm0, rv0, c.ref)
    e_m, e_v = R.row_err(rm.cpu(), want_m), R.row_err(rv.cpu(), want_v)
    print(f"fwd count=1 R={reps}: running mean {e_m:.2e}, running var {e_v:.2e} (bar {ROW_BAR})")
    assert e_m < ROW_BAR and e_v < ROW_BAR


@pytest.mark.parametrize("reps", [1, 9])
def test_finalize_forward_clamp_and_zero(reps):
    """A channel whose Σd²/M is below (Σd/M)² by 1e-3 is clamped to var = 0: invstd = 1/sqrt(eps).
    A set whose sums are all exactly 0 gives the row gamma/sqrt(eps) exactly (a correctly rounded
    sqrt, divide and multiply of fp32 values, as torch-CPU fp32 computes them)."""
    C, M = 70, 16
    gen = torch.Generator().manual_seed(3)
    mean = 0.5 + torch.rand(C, generator=gen, dtype=torch.float64)
    var = 0.5 + torch.rand(C, generator=gen, dtype=torch.float64)
    var[::7] = -1e-3
    c = crafted(mean * M, (var + mean * mean) * M, M, reps)
    t = torch.full((4 * C + GUARD,), NAN, device="cuda")
    finalize(Dev(c).xf(), 0, t)
    tab = check_rows(f"fwd clamp R={reps}", t, C, c.ref, R.FWD_ROWS)
    assert float(c.ref.var[::7].max()) == 0.0 and float(c.ref.var.max()) > 0.4
    e = float((tab[2, ::7].double() * R.EPS ** 0.5 - 1).abs().max())
    print(f"fwd clamp R={reps}: invstd of the clamped channels within {e:.2e} of 1/sqrt(eps) (bar 1e-6)")
    assert e < 1e-6
    z = crafted(torch.zeros(C, dtype=torch.float64), torch.zeros(C, dtype=torch.float64), M, reps, seed=4)
    finalize(Dev(z).xf(), 0, t)
    inv = 1.0 / torch.sqrt(torch.tensor(0.0) + torch.tensor(R.EPS))            # fp32
    got = t[:4 * C].cpu().view(4, C)
    print(f"fwd zero R={reps}: a differs from gamma/sqrt(eps) by at most "
          f"{float((got[0] - z.gamma * inv).abs().max()):.2e}")
    assert torch.equal(got[0], z.gamma * inv)
    assert torch.equal(got[1], z.beta) and torch.equal(got[2], inv.expand(C))
    assert torch.equal(got[3].abs(), torch.zeros(C))


# ------------------------------------------------------------------------------------- (b) mode 1
def start_values(ref, seed):
    """Non-zero start values of the once-only outputs, of each row's own size (a start far larger
    than the addend would hide the addend inside the bar)."""
    gen = torch.Generator().manual_seed(seed)
    scale = sum(x.abs() for x in ref.db_terms)
    return (0.5 * ref.dgamma.abs().max() * torch.randn(ref.dgamma.numel(), generator=gen, dtype=torch.float64),
            0.5 * ref.dbeta.abs().max() * torch.randn(ref.dbeta.numel(), generator=gen, dtype=torch.float64),
            (0.5 * scale * torch.randn(scale.numel(), generator=gen, dtype=torch.float64).clamp(-2, 2)).float().double())


def check_db(tag, got, start, ref, calls=1):
    """|got - start| per channel against DB_BAR · (|A·Σg| + |B·Σy| + |C·M|), each call."""
    scale = sum(x.abs() for x in ref.db_terms)
    e = (got.double() - start.double()).abs() / scale
    vis = R.db_terms_visible(ref, 100.0, DB_BAR)
    print(f"{tag}: db moved by at most {float(e.max()):.2e} of the terms' sum (bar {calls * DB_BAR:.0e}); "
          f"every term >= 100 bars on {100 * vis:.1f} % of the channels")
    assert vis >= 0.98
    assert float(e.max()) <= calls * DB_BAR, tag


@pytest.mark.parametrize("centred", [False, True], ids=["shift", "noshift"])
@pytest.mark.parametrize("C,reps,pad,M", GRID)
def test_finalize_backward(C, reps, pad, M, centred):
    """Mode 1: the [3][C] table; dgamma_out, dbeta_out and db added onto non-zero start values exactly
    once per call; db = NULL or dgamma_out = NULL leaves everything else as it was; the GPU's table
    reproduces autograd's dL/dy."""
    c = grid_case(C, reps, pad, M, centred)
    d, ref = Dev(c), c.ref
    tag = f"bwd C={C} R={reps} rstride={c.rstride} M={M} {'no shift' if centred else 'shift'}"
    s_dg, s_db_, s_bias = start_values(ref, C)
    (dgb, dg), (dbb, db_), (bib, bias) = guarded(s_dg), guarded(s_db_), guarded(s_bias)
    s_dg, s_db_, s_bias = dg.cpu().double(), db_.cpu().double(), bias.cpu().double()      # as stored (fp32)
    x = d.xf()
    x.dgamma_out, x.dbeta_out = dg.data_ptr(), db_.data_ptr()
    t1 = torch.full((3 * C + GUARD,), NAN, device="cuda")
    log = launched(lambda: finalize(x, 1, t1, bias))
    assert "bn_finalize_kernel" in log, log
    tab = check_rows(tag, t1, C, ref, R.BWD_ROWS)
    assert all(guard_intact(b, n) for b, n in ((t1, 3 * C), (dgb, C), (dbb, C), (bib, C)))
    first = bias.cpu().clone()
    for calls in (1, 2):
        if calls == 2:
            finalize(x, 1, t1, bias)
        e_dg = R.row_err(dg.cpu(), s_dg + calls * ref.dgamma)
        e_db = R.row_err(db_.cpu(), s_db_ + calls * ref.dbeta)
        print(f"{tag}: after {calls} call(s) dgamma_out {e_dg:.2e}, dbeta_out {e_db:.2e} (bar {ROW_BAR})")
        assert e_dg < ROW_BAR and e_db < ROW_BAR
    check_db(tag + " call 1", first, s_bias, ref)
    check_db(tag + " call 2", bias.cpu(), first, ref)
    # the optional outputs, one at a time
    keep = [t.clone() for t in (dg, db_, bias)]
    t2 = torch.full((3 * C + GUARD,), NAN, device="cuda")
    finalize(x, 1, t2)                                        # db = NULL
    assert torch.equal(t2[:3 * C], t1[:3 * C]) and torch.equal(bias, keep[2])
    assert R.row_err(dg.cpu(), s_dg + 3 * ref.dgamma) < ROW_BAR and R.row_err(db_.cpu(), s_db_ + 3 * ref.dbeta) < ROW_BAR
    x.dgamma_out = None
    keep = [t.clone() for t in (dg, db_, bias)]
    t3 = torch.full((3 * C + GUARD,), NAN, device="cuda")
    finalize(x, 1, t3, bias)                                  # dgamma_out = NULL
    assert torch.equal(t3[:3 * C], t1[:3 * C]) and torch.equal(dg, keep[0])
    assert R.row_err(db_.cpu(), s_db_ + 4 * ref.dbeta) < ROW_BAR
    check_db(tag + " dgamma_out NULL", bias.cpu(), keep[2].cpu(), ref)
    # dy = A g + B y + C with the GPU's table against autograd
    tabd = tab.double()
    _, dy = R.autograd_dy(c)
    e_dy = R.row_err(tabd[0][None] * c.g + tabd[1][None] * c.y + tabd[2][None], dy)
    print(f"{tag}: A g + B y + C from the GPU's table against autograd {e_dy:.2e} (bar {ROW_BAR})")
    assert e_dy < ROW_BAR


# ------------------------------------------------------------------------------------- (c) mode 2
@pytest.mark.parametrize("C", [3, 130, 4096])
def test_finalize_eval(C):
    """Mode 2: the forward table from the running statistics is eval-mode F.batch_norm (C = 130: two
    channels past the first 128; C = 4096: the 257-th channel takes the second workgroup); the running
    buffers are unchanged bit for bit."""
    c = R.make_case(C, 1, 8)
    d = Dev(c)
    rm0, rv0 = random_running(C, 17 + C)
    (rmb, rm), (rvb, rv) = guarded(rm0), guarded(rv0)
    x = d.xf()
    x.running_mean, x.running_var = rm.data_ptr(), rv.data_ptr()
    t = torch.full((4 * C + GUARD,), NAN, device="cuda")
    log = launched(lambda: finalize(x, 2, t))
    assert "bn_eval_table_kernel" in log and "bn_finalize_kernel" not in log, log
    invstd = 1.0 / torch.sqrt(rv0.double() + R.EPS)
    a = c.gamma.double() * invstd
    ref = SimpleNamespace(a=a, b=c.beta.double() - rm0.double() * a, p=invstd, q=-rm0.double() * invstd)
    tab = check_rows(f"eval C={C}", t, C, ref, R.FWD_ROWS).double()
    want = F.batch_norm(c.y, rm0.double(), rv0.double(), c.gamma.double(), c.beta.double(), False, R.MOMENTUM, R.EPS)
    e = R.row_err(tab[0][None] * c.y + tab[1][None], want)
    print(f"eval C={C}: a y + b against F.batch_norm(training=False) {e:.2e} (bar {ROW_BAR})")
    assert e < ROW_BAR
    assert torch.equal(rm.cpu(), rm0) and torch.equal(rv.cpu(), rv0)
    assert guard_intact(t, 4 * C) and guard_intact(rmb, C) and guard_intact(rvb, C)


# ------------------------------------------------------------------------------------- (d) refusals
REFUSALS = ["reps33", "mode3", "mode-1", "eval_no_running", "bwd_no_dgamma", "count0", "channels0", "no_table"]


@pytest.mark.parametrize("what", REFUSALS)
def test_finalize_refuses(what):
    L = _L()
    c = R.make_case(24, 5, 192, rstride=32)
    d = Dev(c)
    x = d.xf()
    rm, rv = torch.zeros(24, device="cuda"), torch.ones(24, device="cuda")
    table = torch.full((4 * 24,), NAN, device="cuda")
    a = L.BnArgs(mode=0)
    a.table = table.data_ptr()
    if what == "reps33":
        x.reps = 33
    elif what == "mode3":
        a.mode = 3
    elif what == "mode-1":
        a.mode = -1
    elif what == "eval_no_running":
        a.mode = 2
    elif what == "bwd_no_dgamma":
        a.mode = 1
        x.dgamma = None
    elif what == "count0":
        x.count = 0.0
    elif what == "channels0":
        x.channels = 0
    elif what == "no_table":
        a.table = None
    a.xf = x

    def run():
        with pytest.raises(L.VaeHipError):
            L.call("vae_bn_finalize", ctypes.byref(a), _stream())
    log = launched(run)
    torch.cuda.synchronize()
    assert log.strip() == "", log
    assert torch.isnan(table).all()
    # the same arguments without the defect are accepted (the refusal is about the defect)
    ok = L.BnArgs(mode=0)
    x2 = d.xf()
    x2.running_mean, x2.running_var = rm.data_ptr(), rv.data_ptr()
    ok.xf, ok.table = x2, table.data_ptr()
    L.call("vae_bn_finalize", ctypes.byref(ok), _stream())
    torch.cuda.synchronize()
    assert torch.isfinite(table).all()


# ------------------------------------------------------------------------ (e), (f) vae_bn_apply
def bf16(t):
    return t.to(torch.bfloat16)


def apply_rows(C):
    """Rows so that rows·C/8 > 1024 chunks: at least two workgroups of 256 threads x 4 chunks."""
    rows = 8192 // C + 8
    assert rows * C // 8 > 1024
    return rows


def bn_apply(src, x, out, db=None):
    L = _L()
    a = L.BnApplyArgs(dtype=L.BF16, rows=src.shape[0], channels=src.shape[1])
    a.x, a.xf, a.out = src.data_ptr(), x, out.data_ptr()
    if db is not None:
        a.db = db.data_ptr()
    log = launched(lambda: L.call("vae_bn_apply", ctypes.byref(a), _stream()))
    torch.cuda.synchronize()
    assert "bn_apply_kernel" in log, log
    return log


def check_out(tag, out, ref, slack=None):
    """|out - ref| <= 2^-8 · |ref| (+ slack) elementwise, ref the fp64 value before its bf16 rounding.

    2^-8 · |ref| is half a bf16 ulp at the bottom of a binade — the most a correctly rounded bf16 can
    be away from the value it rounds.  Held against the unrounded reference: fp32 arithmetic that is
    1e-7 from fp64 lands on the other side of a rounding tie on about one element in 10^4, and out then
    differs from bf16(ref) by a whole ulp (up to 2^-7 · |ref|) while still being the nearest bf16 of a
    value 1e-7 from ref.  An fp32 CPU emulation of the kernel's arithmetic shows such flips in 4 of
    these 26 cases and no element over this bar; the flips are counted and printed."""
    got = out.cpu().double()
    err = (got - ref).abs()
    bar = 2.0 ** -8 * ref.abs() + (0 if slack is None else slack)
    over = err > bar
    worst = float((err / bar.clamp_min(1e-300)).max())
    flips = got != ref.to(torch.bfloat16).double()
    print(f"{tag}: worst |out - ref| is {worst:.3f} of the elementwise bar, {int(over.sum())} of {over.numel()} "
          f"elements over it; {int(flips.sum())} elements are not bf16(ref)")
    assert not bool(over.any()), (tag, int(over.sum()))


def apply_case(C, reps):
    return R.make_case(C, reps, apply_rows(C), rstride=C + 8 if reps > 1 else None, seed=1)


def conditioned(tag, y, ref):
    """The stored bf16 operand of a BN_ACT check: bf16(y), with the elements whose a·y and b cancel
    below 2^-8 of |a·y| + |b| scaled by 1 + 2^-4 (which leaves |z| near 2^-5 of that sum).

    The bar on the output is purely relative to |ref| = |lrelu(a·y + b)|.  The table holds a and b in
    fp32, a few 2^-24 each, so z = a·y + b carries about 2^-21 · (|a·y| + |b|) whatever the kernel
    does; where the two cancel by 2^-13 or more that alone is the whole bar (and near z = 0 it picks
    the other LeakyReLU branch).  Measured: one such element at C = 1032, a·y = -0.395452,
    b = 0.395471, z = 1.9e-5, out 1.14 bars away on the GPU and in an fp32 emulation on the CPU alike.
    Decided from the fp64 reference alone; the statistics are inputs of their own and do not move."""
    yb = bf16(y)
    yd = yb.double()
    ay, b = ref.a[None] * yd, ref.b[None]
    bad = (ay + b).abs() < 2.0 ** -8 * (ay.abs() + b.abs())
    yb = torch.where(bad, bf16(yd * (1 + 2.0 ** -4)), yb)
    print(f"{tag}: {int(bad.sum())} of {bad.numel()} elements moved off a cancelling a·y + b")
    return yb


def run_apply_act(tag, c, x, table_ref):
    yb = conditioned(tag, c.y, table_ref).cuda()
    out = torch.full((c.M * c.C + GUARD,), NAN, device="cuda", dtype=torch.bfloat16)
    bn_apply(yb, x, out)
    ref = F.leaky_relu(table_ref.a[None] * yb.cpu().double() + table_ref.b[None], R.SLOPE)
    check_out(tag, out[:c.M * c.C].view(c.M, c.C), ref)
    assert guard_intact(out.float(), c.M * c.C)


def run_apply_dy(tag, c, x, table_ref, db=None):
    yb, gb = bf16(c.y).cuda(), bf16(c.g).cuda()
    x.aux = yb.data_ptr()
    out = torch.full((c.M * c.C + GUARD,), NAN, device="cuda", dtype=torch.bfloat16)
    bn_apply(gb, x, out, db)
    yd, gd = yb.cpu().double(), gb.cpu().double()
    A, B, Cc = table_ref.A[None], table_ref.B[None], table_ref.C[None]
    ref = A * gd + B * yd + Cc
    check_out(tag, out[:c.M * c.C].view(c.M, c.C), ref, DB_BAR * ((A * gd).abs() + (B * yd).abs() + Cc.abs()))
    assert guard_intact(out.float(), c.M * c.C)


FAST = [(64, 4), (8, 32), (256, 4), (128, 8), (512, 1), (512, 2)]           # bn_fast_ok: one round of loads
PLAIN = [(96, 1), (24, 5), (1024, 1), (128, 9), (512, 3), (64, 32), (64, 17)]  # the plain loop (rsum)


@pytest.mark.parametrize("C,reps", FAST + PLAIN)
def test_bn_apply_builds_the_forward_table(C, reps):
    """BN_ACT with xf.table = NULL: lrelu(a y + b) from the statistics, and the running statistics
    updated exactly once although two or more workgroups build the table."""
    L = _L()
    c = apply_case(C, reps)
    d = Dev(c)
    tag = f"apply BN_ACT C={C} R={reps} rows={c.M}"
    rm0, rv0 = random_running(C, 3 * C + reps)
    (rmb, rm), (rvb, rv) = guarded(rm0), guarded(rv0)
    x = d.xf(L.X_BN_ACT)
    x.running_mean, x.running_var = rm.data_ptr(), rv.data_ptr()
    run_apply_act(tag, c, x, c.ref)
    want_m, want_v = R.running_update(rm0, rv0, c.ref)
    e_m, e_v = R.row_err(rm.cpu(), want_m), R.row_err(rv.cpu(), want_v)
    print(f"{tag}: running mean {e_m:.2e}, running var {e_v:.2e} (bar {ROW_BAR})")
    assert e_m < ROW_BAR and e_v < ROW_BAR
    assert guard_intact(rmb, C) and guard_intact(rvb, C)


@pytest.mark.parametrize("C,reps", FAST + PLAIN)
def test_bn_apply_builds_the_backward_table(C, reps):
    """BN_DY with xf.table = NULL: A g + B y + C from the statistics; dgamma_out, dbeta_out and db
    accumulated exactly once (closed_form_db in the first workgroup); running statistics untouched."""
    L = _L()
    c = apply_case(C, reps)
    d, ref = Dev(c), c.ref
    tag = f"apply BN_DY C={C} R={reps} rows={c.M}"
    s_dg, s_db_, s_bias = start_values(ref, C + 1)
    (dgb, dg), (dbb, db_), (bib, bias) = guarded(s_dg), guarded(s_db_), guarded(s_bias)
    s_dg, s_db_, s_bias = dg.cpu().double(), db_.cpu().double(), bias.cpu().double()
    rm0, rv0 = random_running(C, 9)
    (rmb, rm), (rvb, rv) = guarded(rm0), guarded(rv0)
    x = d.xf(L.X_BN_DY)
    x.dgamma_out, x.dbeta_out = dg.data_ptr(), db_.data_ptr()
    x.running_mean, x.running_var = rm.data_ptr(), rv.data_ptr()
    run_apply_dy(tag, c, x, ref, bias)
    e_dg, e_db = R.row_err(dg.cpu(), s_dg + ref.dgamma), R.row_err(db_.cpu(), s_db_ + ref.dbeta)
    print(f"{tag}: dgamma_out {e_dg:.2e}, dbeta_out {e_db:.2e} (bar {ROW_BAR})")
    assert e_dg < ROW_BAR and e_db < ROW_BAR
    check_db(tag, bias.cpu(), s_bias, ref)
    assert torch.equal(rm.cpu(), rm0) and torch.equal(rv.cpu(), rv0)
    assert all(guard_intact(b, C) for b in (dgb, dbb, bib, rmb, rvb))


@pytest.mark.parametrize("C", [256, 1032, 4096])
def test_bn_apply_copies_a_finalized_table(C):
    """Both kinds with xf.table written by vae_bn_finalize (C = 1032: one full 1024-channel round of
    the copy and a tail of 8; C = 4096: four rounds); with a table set the running statistics, the
    affine gradients and db are vae_bn_finalize's business and do not move."""
    L = _L()
    c = R.make_case(C, 4 if C == 256 else 2, apply_rows(C), rstride=C + 8, seed=2)
    d = Dev(c)
    tf = torch.full((4 * C + GUARD,), NAN, device="cuda")
    tb = torch.full((3 * C + GUARD,), NAN, device="cuda")
    finalize(d.xf(), 0, tf)
    finalize(d.xf(), 1, tb)
    b = tb[:3 * C].cpu().double().view(3, C)
    check_rows(f"table C={C}", tf, C, c.ref, R.FWD_ROWS)
    check_rows(f"table C={C}", tb, C, c.ref, R.BWD_ROWS)
    rm0, rv0 = random_running(C, 1)
    rm, rv = rm0.cuda(), rv0.cuda()
    x = d.xf(L.X_BN_ACT)
    x.table, x.running_mean, x.running_var = tf.data_ptr(), rm.data_ptr(), rv.data_ptr()
    # the reference is the fp64 table: the copied fp32 table is within ROW_BAR of it, far inside a bf16 ulp
    run_apply_act(f"apply BN_ACT table C={C}", c, x, c.ref)
    assert torch.equal(rm.cpu(), rm0) and torch.equal(rv.cpu(), rv0)
    x = d.xf(L.X_BN_DY)
    x.table, x.running_mean, x.running_var = tb.data_ptr(), rm.data_ptr(), rv.data_ptr()
    run_apply_dy(f"apply BN_DY table C={C}", c, x, c.ref)
    assert torch.equal(rm.cpu(), rm0) and torch.equal(rv.cpu(), rv0)
    # ... and exactly the table's values reach the output: the same call on the GPU's own fp32 rows
    yb, gb = bf16(c.y).cuda(), bf16(c.g).cuda()
    x.aux = yb.data_ptr()
    out = torch.empty(c.M, C, device="cuda", dtype=torch.bfloat16)
    bn_apply(gb, x, out)
    gd, yd = gb.cpu().double(), yb.cpu().double()
    ref = b[0][None] * gd + b[1][None] * yd + b[2][None]
    check_out(f"apply BN_DY own table C={C}", out, ref,
              DB_BAR * ((b[0][None] * gd).abs() + (b[1][None] * yd).abs() + b[2][None].abs()))


# --------------------------------------------------------------- (g) producer -> finalisation chains
@pytest.mark.parametrize("reps", [1, 4, 8])
def test_conv_fwd_then_finalize(reps):
    """vae_conv2d_fwd (16 -> 48, 12 x 12, N = 4, fp32) leaves its statistics in `reps` replicas
    cout + 8 floats apart and carries a mode-0 finalisation: the fused table is fp64 BatchNorm of the
    fp64 conv output (10 tol(fp32): the conv's own error goes in), a separate vae_bn_finalize launch on
    the same sums writes the same bits, and the running statistics are nn.BatchNorm2d's."""
    L = _L()
    torch.manual_seed(0)
    N, cin, cout, hw, dtype = 4, 16, 48, 12, torch.float32
    x = torch.randn(N, cin, hw, hw)
    w = torch.randn(cout, cin, 3, 3) * 0.1
    b = torch.randn(cout) * 0.1
    gamma, beta = 0.8 + 0.4 * torch.rand(cout), torch.rand(cout) * 0.2 - 0.1
    rm0, rv0 = random_running(cout, 2)
    y64 = F.conv2d(x.double(), w.double(), b.double(), stride=2, padding=1)
    bn = torch.nn.BatchNorm2d(cout, eps=R.EPS, momentum=R.MOMENTUM).double()
    with torch.no_grad():
        bn.weight.copy_(gamma); bn.bias.copy_(beta); bn.running_mean.copy_(rm0); bn.running_var.copy_(rv0)
    bn.train()
    bn(y64)
    mean, var = y64.mean((0, 2, 3)), y64.var((0, 2, 3), unbiased=False)
    invstd = 1.0 / torch.sqrt(var + R.EPS)
    ref = SimpleNamespace(a=gamma.double() * invstd, b=beta.double() - mean * gamma.double() * invstd, p=invstd,
                          q=-mean * invstd)
    rs = cout + 8
    sums = torch.zeros(2, max(1, reps), rs, device="cuda")
    sums[:, :, cout:] = NAN
    out = torch.empty(N, hw // 2, hw // 2, cout, device="cuda", dtype=dtype)
    xd, wd, bd = nhwc(x, dtype), w.permute(0, 2, 3, 1).contiguous().cuda(), b.cuda()
    gd, bed = gamma.cuda(), beta.cuda()
    (rmb, rm), (rvb, rv) = guarded(rm0), guarded(rv0)
    P = hw // 2
    xf = L.Xform(kind=L.X_BN_ACT, channels=cout, slope=R.SLOPE, count=float(N * P * P), eps=R.EPS, momentum=R.MOMENTUM)
    xf.sum, xf.sumsq, xf.shift = sums[0].data_ptr(), sums[1].data_ptr(), bd.data_ptr()
    xf.gamma, xf.beta = gd.data_ptr(), bed.data_ptr()
    xf.reps, xf.rstride = reps, (rs if reps > 1 else 0)
    xf.running_mean, xf.running_var = rm.data_ptr(), rv.data_ptr()
    fused = torch.full((4 * cout + GUARD,), NAN, device="cuda")
    fin = L.BnArgs(mode=0)
    fin.xf, fin.table = xf, fused.data_ptr()
    a = L.ConvArgs(dtype=L.dtype_code(dtype), n=N, h=hw, w=hw, c=cin, k=cout, p=P, q=P, r=3, stride=2, pad=1)
    a.x = xd.data_ptr(); a.wt = wd.data_ptr(); a.bias = bd.data_ptr(); a.y = out.data_ptr()
    a.y_sum, a.y_sumsq = sums[0].data_ptr(), sums[1].data_ptr()
    a.sum_reps, a.sum_rstride = reps, (rs if reps > 1 else 0)
    a.bn_finalize = ctypes.pointer(fin)
    ws = give_workspace(a, "vae_conv2d_fwd")
    log = launched(lambda: L.call("vae_conv2d_fwd", ctypes.byref(a), _stream()))
    torch.cuda.synchronize()
    assert "bn_finalize_kernel" in log, log
    t = tol(dtype)
    assert rel(to_nchw(out), y64.float()) < t
    used = int((sums[0, :, :cout].abs().sum(1) > 0).sum())
    tab = fused[:4 * cout].cpu().view(4, cout)
    errs = {k: R.row_err(tab[i], getattr(ref, k)) for i, k in enumerate(R.FWD_ROWS)}
    e_m = R.row_err(rm.cpu(), bn.running_mean)
    e_v = R.row_err(rv.cpu(), bn.running_var)
    print(f"conv -> finalize R={reps} ({used} replicas written): " + ", ".join(f"{k} {e:.2e}" for k, e in errs.items()) +
          f", running mean {e_m:.2e}, running var {e_v:.2e} (bar {10 * t:.0e})")
    assert max(errs.values()) < 10 * t and e_m < 10 * t and e_v < 10 * t
    assert guard_intact(fused, 4 * cout) and guard_intact(rmb, cout) and guard_intact(rvb, cout)
    sep = torch.full((4 * cout + GUARD,), NAN, device="cuda")
    xf.running_mean = xf.running_var = None
    finalize(xf, 0, sep)
    assert torch.equal(sep[:4 * cout], fused[:4 * cout])


@pytest.mark.parametrize("reps", [1, 4])
def test_conv_bwd_data_then_finalize(reps):
    """The setup of test_gpu_ops.test_conv2d_backward_bn in fp32: vae_conv2d_bwd_data leaves Σg·x̂, Σg of
    the previous BatchNorm in `reps` replicas and carries mode 1 on that BatchNorm (a.bn_finalize); a
    separate vae_bn_finalize launch on the same sums writes the same bits; A·dx + B·y_prev + C is
    autograd's y_prev.grad within 20 tol(fp32), that test's bar for the BatchNorm parameter gradients."""
    L = _L()
    from gpu_util import BNState
    dtype = torch.float32
    torch.manual_seed(4)
    N, cin, cout, hw = 4, 32, 64, 8
    y_prev = (torch.randn(N, cin, hw, hw) * 1.2 + 0.2).requires_grad_()
    g_prev = 0.8 + 0.4 * torch.rand(cin); b_prev = torch.rand(cin) * 0.2 - 0.1
    gp = g_prev.clone().requires_grad_(); bp = b_prev.clone().requires_grad_()
    a_prev = F.leaky_relu(F.batch_norm(y_prev, None, None, gp, bp, True, 0.1, 1e-5), 0.01)
    w = (torch.randn(cout, cin, 3, 3) * 0.1).requires_grad_()
    bias = (torch.randn(cout) * 0.1).requires_grad_()
    y = F.conv2d(a_prev, w, bias, stride=2, padding=1)
    g_cur = 0.8 + 0.4 * torch.rand(cout); b_cur = torch.rand(cout) * 0.2 - 0.1
    z = F.batch_norm(y, None, None, g_cur, b_cur, True, 0.1, 1e-5)
    gz = torch.randn_like(z)
    z.backward(gz)
    bnp = BNState(y_prev.detach(), dtype=dtype); bnp.gamma, bnp.beta = g_prev, b_prev
    bnp.dev["gamma"], bnp.dev["beta"] = g_prev.cuda(), b_prev.cuda()
    yv = y.detach()
    bnc = BNState(yv, shift=bias.detach(), dtype=dtype); bnc.gamma, bnc.beta = g_cur, b_cur
    bnc.dev["gamma"], bnc.dev["beta"] = g_cur.cuda(), b_cur.cuda()
    mean = yv.mean((0, 2, 3), keepdim=True); var = yv.var((0, 2, 3), unbiased=False, keepdim=True)
    xh = (yv - mean) / torch.sqrt(var + 1e-5)
    dgam = (gz * xh).sum((0, 2, 3)).cuda(); dbet = gz.sum((0, 2, 3)).cuda()
    gzd = nhwc(gz, dtype)
    wd = w.detach().permute(0, 2, 3, 1).contiguous().to("cuda", dtype)
    dx = torch.empty(N, hw, hw, cin, device="cuda", dtype=dtype)
    rs = cin + 8
    sums = torch.zeros(2, max(1, reps), rs, device="cuda")              # Σg·x̂ | Σg of the previous BatchNorm
    sums[:, :, cin:] = NAN
    a = L.ConvArgs(dtype=L.dtype_code(dtype), n=N, h=hw, w=hw, c=cin, k=cout, p=hw // 2, q=hw // 2, r=3, stride=2, pad=1)
    a.dy = gzd.data_ptr()
    a.dy_xf = bnc.xf(L.X_BN_DY, aux=bnc.y_dev, dgamma=dgam, dbeta=dbet)
    a.wt = wd.data_ptr()
    a.dx = dx.data_ptr()
    a.dx_epi = bnp.xf(L.X_BN_ACT, aux=bnp.y_dev)
    a.dx_dgamma, a.dx_dbeta = sums[0].data_ptr(), sums[1].data_ptr()
    a.sum_reps, a.sum_rstride = reps, (rs if reps > 1 else 0)
    # mode 1 on the previous BatchNorm from the sums this call leaves; one descriptor carries one
    # replica layout, so its forward sums are laid out like the backward ones
    gen = torch.Generator().manual_seed(reps)
    fs, fq = (R.split_replicas(v, reps, rs, gen).cuda() for v in (bnp.sum, bnp.sumsq))

    def mode1():
        xf = bnp.xf(L.X_BN_DY, dgamma=sums[0], dbeta=sums[1])
        xf.sum, xf.sumsq = fs.data_ptr(), fq.data_ptr()
        xf.reps, xf.rstride = reps, (rs if reps > 1 else 0)
        dgo, dbo = torch.zeros(cin, device="cuda"), torch.zeros(cin, device="cuda")
        xf.dgamma_out, xf.dbeta_out = dgo.data_ptr(), dbo.data_ptr()
        table = torch.full((3 * cin + GUARD,), NAN, device="cuda")
        fin = L.BnArgs(mode=1)
        fin.xf, fin.table = xf, table.data_ptr()
        return fin, table, dgo, dbo
    fin_f, tab_f, dgo_f, dbo_f = mode1()
    fin_s, tab_s, dgo_s, dbo_s = mode1()
    a.bn_finalize = ctypes.pointer(fin_f)
    ws = give_workspace(a, "vae_conv2d_bwd_data")
    log = launched(lambda: L.call("vae_conv2d_bwd_data", ctypes.byref(a), _stream()))
    torch.cuda.synchronize()
    assert "bn_finalize_kernel" in log, log
    L.call("vae_bn_finalize", ctypes.byref(fin_s), _stream())
    torch.cuda.synchronize()
    assert torch.equal(tab_f[:3 * cin], tab_s[:3 * cin]) and torch.equal(dgo_f, dgo_s) and torch.equal(dbo_f, dbo_s)
    assert guard_intact(tab_f, 3 * cin) and guard_intact(tab_s, 3 * cin)
    used = int((sums[1, :, :cin].abs().sum(1) > 0).sum())
    t = tol(dtype)
    e_dg, e_db = rel(dgo_f.cpu(), gp.grad), rel(dbo_f.cpu(), bp.grad)
    tab = tab_f[:3 * cin].cpu().double().view(3, cin)
    v = lambda r: tab[r].view(1, -1, 1, 1)
    mine = v(0) * to_nchw(dx).double() + v(1) * y_prev.detach().double() + v(2)
    e_dy = rel(mine, y_prev.grad)
    print(f"dgrad -> finalize R={reps} ({used} replicas written): dgamma {e_dg:.2e}, dbeta {e_db:.2e}, "
          f"A dx + B y + C against autograd {e_dy:.2e} (bar {20 * t:.0e})")
    assert e_dg < 20 * t and e_db < 20 * t and e_dy < 20 * t
