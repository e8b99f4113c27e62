"""Train-mode BatchNorm as the library computes it, restated in plain torch for the tests.

The library never runs BatchNorm as an op: a producer leaves replicated per-channel sums
Σ(y - shift), Σ(y - shift)² (forward) and Σg·x̂, Σg (backward), and every consumer works from a
per-channel coefficient table (include/vaehip.h vae_xform.table):

    forward   z = a·y + b,  x̂ = p·y + q        a = γ·invstd, b = β - mean·a, p = invstd, q = -mean·invstd
    backward  dy = A·g + B·y + C               A = γ·invstd, B = -A·invstd·Σg·x̂/M,
                                               C = -A·(Σg/M - mean·invstd·Σg·x̂/M)

`bn_tables` is that arithmetic from the replicated statistics, in any dtype (fp64: the reference the
GPU builders are held to; fp32: what a correct fp32 builder can reach).  tests/test_bn_ref.py pins it
against torch's own batch_norm, BatchNorm2d and autograd in fp64.

`make_case` makes the small real tensors of the issue's input recipe and their replicated statistics
(`split_replicas`: R unequal rows `rstride` floats apart, the pad floats NaN)."""
import functools
from types import SimpleNamespace

import torch

EPS, MOMENTUM, SLOPE = 1e-5, 0.1, 0.01


def split_replicas(total, reps, rstride, gen, dtype=torch.float32):
    """A [C] total as `reps` unequal fp32 replica rows, `rstride` floats apart: [reps, max(rstride, C)],
    row r = w_r · total with random weights that sum to 1 (one of them negative when reps > 1), the
    floats between the rows NaN.  reps = 1: the total itself (rstride may be 0).  dtype: fp32 as the
    kernels read them; fp64 where a test pins the arithmetic itself."""
    C = total.numel()
    reps = max(1, reps)
    width = C if reps == 1 else rstride
    assert width >= C, (rstride, C)
    w = 0.5 + torch.rand(reps, generator=gen, dtype=torch.float64)
    if reps > 1:
        w[int(torch.randint(reps, (1,), generator=gen))] = -0.25
    w = w / w.sum()
    out = torch.full((reps, width), float("nan"), dtype=dtype)
    out[:, :C] = (w[:, None] * total.double()[None, :]).to(dtype)
    return out


def replica_rows(buf, C):
    """The [R, C] statistics of a split_replicas buffer (pads dropped)."""
    return buf[:, :C]


def bn_tables(sum_r, sumsq_r, dgamma_r, dbeta_r, shift, gamma, beta, count, eps=EPS, dtype=torch.float64):
    """Every per-channel quantity the builders derive, from the replicated statistics [R, C] as the
    kernels read them (dgamma_r / dbeta_r / shift may be None).  Computed in `dtype` throughout."""
    cv = lambda t: None if t is None else t.to(dtype)
    s, ss = cv(sum_r).sum(0), cv(sumsq_r).sum(0)
    gamma, beta = cv(gamma), cv(beta)
    sh = torch.zeros_like(s) if shift is None else cv(shift)
    M = torch.tensor(float(count), dtype=dtype)
    s1 = s / M
    var = (ss / M - s1 * s1).clamp_min(0)
    mean = s1 + sh
    invstd = 1.0 / torch.sqrt(var + torch.tensor(eps, dtype=dtype))
    unb = var * M / (M - 1) if count > 1 else var
    a = gamma * invstd
    t = SimpleNamespace(mean=mean, var=var, unb=unb, invstd=invstd, a=a, b=beta - mean * a, p=invstd,
                        q=-mean * invstd, count=count)
    if dgamma_r is not None:
        dgam, dbet = cv(dgamma_r).sum(0), cv(dbeta_r).sum(0)
        mgx, mg = dgam / M, dbet / M
        A = a
        B = -A * invstd * mgx
        C = -A * (mg - mean * invstd * mgx)
        t.A, t.B, t.C, t.dgamma, t.dbeta = A, B, C, dgam, dbet
        # the closed-form gradient of a bias in front of the BatchNorm, Σ dy = A·Σg + B·Σy + C·M, by term
        t.db_terms = (A * dbet, B * (s + M * sh), C * M)
    return t


def running_update(start_mean, start_var, t, momentum=MOMENTUM):
    """torch's running-statistic update (unbiased variance) from a bn_tables result."""
    dt = t.mean.dtype
    return ((1 - momentum) * start_mean.to(dt) + momentum * t.mean,
            (1 - momentum) * start_var.to(dt) + momentum * t.unb)


FWD_ROWS = ("a", "b", "p", "q")
BWD_ROWS = ("A", "B", "C")


@functools.lru_cache(maxsize=None)
def make_case(C, R, M, rstride=None, centred=False, seed=0, stat_dtype=torch.float32):
    """One BatchNorm's tensors by the recipe — y [M, C] = randn·1.5 + 0.3 + a per-channel offset randn,
    shift = channel mean + randn·0.1, gamma = 0.8 + 0.4·rand, g = randn·0.01 — with the fp32
    replicated statistics a producer would leave (R rows, `rstride` apart; default C) and the fp64
    tables from exactly those statistics.  centred: no per-channel offset and no shift (sums taken
    against 0 stay conditioned).  Cached: treat every tensor as read-only."""
    gen = torch.Generator().manual_seed(1000 * C + 10 * R + M + 7919 * seed)
    rn = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)
    y = rn(M, C) * 1.5 + 0.3
    if not centred:
        y = y + rn(C)[None, :]
    g = rn(M, C) * 0.01
    gamma = (0.8 + 0.4 * torch.rand(C, generator=gen, dtype=torch.float64)).float()
    beta = ((torch.rand(C, generator=gen, dtype=torch.float64) * 2 - 1) * 0.1).float()
    shift = None if centred else (y.mean(0) + rn(C) * 0.1).float()
    return case_from(y, g, gamma, beta, shift, R, C if rstride is None else rstride, gen, stat_dtype)


def case_from(y, g, gamma, beta, shift, R, rstride, gen, stat_dtype=torch.float32):
    """The statistics of y [M, C] / g [M, C] (fp64 sums, split into fp32 replicas) and their tables."""
    M, C = y.shape
    y, g = y.double(), g.double()
    d = y if shift is None else y - shift.double()[None, :]
    xhat = (y - y.mean(0)) / torch.sqrt(y.var(0, unbiased=False) + EPS)
    bufs = {k: split_replicas(v, R, rstride, gen, stat_dtype) for k, v in
            (("sum", d.sum(0)), ("sumsq", (d * d).sum(0)), ("dgamma", (g * xhat).sum(0)), ("dbeta", g.sum(0)))}
    rows = {k: replica_rows(v, C) for k, v in bufs.items()}
    ref = bn_tables(rows["sum"], rows["sumsq"], rows["dgamma"], rows["dbeta"], shift, gamma, beta, M)
    return SimpleNamespace(C=C, R=max(1, R), M=M, rstride=(rstride if R > 1 else 0), y=y, g=g, gamma=gamma, beta=beta,
                           shift=shift, bufs=bufs, rows=rows, ref=ref)


def autograd_dy(case):
    """(z, dL/dy) of fp64 F.batch_norm(training=True) on the case's y with upstream gradient g."""
    yv = case.y.clone().requires_grad_(True)
    z = torch.nn.functional.batch_norm(yv, None, None, case.gamma.double(), case.beta.double(), True, MOMENTUM, EPS)
    z.backward(case.g)
    return z.detach(), yv.grad


def row_err(got, want):
    """max |got - want| relative to the row's max-abs (the bar's form for table rows)."""
    got, want = got.double().flatten(), want.double().flatten()
    return float((got - want).abs().max() / want.abs().max().clamp_min(1e-300))


def db_terms_visible(t, factor=100.0, bar=1e-6):
    """Fraction of channels on which each of the three closed-form bias-gradient terms alone is at
    least `factor` times the bias-gradient bar (bar · the three magnitudes' sum)."""
    scale = sum(x.abs() for x in t.db_terms)
    ok = torch.stack([x.abs() >= factor * bar * scale for x in t.db_terms]).all(0)
    return float(ok.double().mean())
