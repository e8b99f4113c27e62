"""Pin the BatchNorm restatement (tests/bn_ref.py) against torch itself in fp64, and show that the
bars of tests/test_gpu_bn_tables.py are reachable by a correct fp32 builder.

Bars.  With fp64 replicas the restatement and torch differ only by fp64 rounding through a variance
whose two terms nearly cancel (Σd²/M against (Σd/M)², |d| a few units): 1e-10 of each tensor's max
leaves four orders of margin and is five below the first wrong digit of any formula error.  With the
fp32 replicas the GPU tests hand to the kernels, the statistics themselves carry 2^-24 relative
rounding per replica: the figure against autograd is printed and held to 1e-6, a tenth of the GPU bar."""
import pytest
import torch
import torch.nn.functional as F

import bn_ref as R

CASES = [(24, 5, 192), (64, 4, 192), (96, 1, 32), (512, 2, 20), (1000, 32, 8), (4096, 1, 8)]   # C, reps, M


def _case(C, reps, M, dt):
    return R.make_case(C, reps, M, rstride=C + 8 if reps > 1 else None, stat_dtype=dt)


@pytest.mark.parametrize("C,reps,M", CASES)
def test_forward_and_backward_are_torch(C, reps, M):
    c = _case(C, reps, M, torch.float64)
    t = c.ref
    z, dy = R.autograd_dy(c)
    e_z = R.row_err(t.a[None] * c.y + t.b[None], z)
    e_xh = R.row_err(t.p[None] * c.y + t.q[None], (c.y - c.y.mean(0)) / torch.sqrt(c.y.var(0, unbiased=False) + R.EPS))
    mine = t.A[None] * c.g + t.B[None] * c.y + t.C[None]
    e_dy = R.row_err(mine, dy)
    e_var = R.row_err(t.var, c.y.var(0, unbiased=False))
    e_mean = R.row_err(t.mean, c.y.mean(0))
    print(f"C={C} R={reps} M={M}: z {e_z:.1e} xhat {e_xh:.1e} dy {e_dy:.1e} mean {e_mean:.1e} var {e_var:.1e}")
    assert max(e_z, e_xh, e_dy, e_mean, e_var) < 1e-10
    # a train-mode BatchNorm's input gradient sums to zero over the batch, term by term of the closed form
    scale = sum(x.abs() for x in t.db_terms)
    assert float((mine.sum(0).abs() / scale).max()) < 1e-10
    assert float((sum(t.db_terms).abs() / scale).max()) < 1e-10
    # ... and the same from the fp32 replicas the kernels read
    c32 = _case(C, reps, M, torch.float32)
    t32 = c32.ref
    e32 = R.row_err(t32.A[None] * c32.g + t32.B[None] * c32.y + t32.C[None], dy)
    print(f"    fp32 replicas, fp64 arithmetic: dy against autograd {e32:.1e}")
    assert e32 < 1e-6


@pytest.mark.parametrize("start", ["default", "random"])
@pytest.mark.parametrize("C,reps,M", CASES)
def test_running_statistics_are_batchnorm2d(C, reps, M, start):
    c = _case(C, reps, M, torch.float64)
    bn = torch.nn.BatchNorm2d(C, eps=R.EPS, momentum=R.MOMENTUM).double()
    if start == "random":
        gen = torch.Generator().manual_seed(C)
        with torch.no_grad():
            bn.running_mean.copy_(torch.randn(C, generator=gen, dtype=torch.float64))
            bn.running_var.copy_(0.5 + torch.rand(C, generator=gen, dtype=torch.float64))
    rm0, rv0 = bn.running_mean.clone(), bn.running_var.clone()
    bn.train()
    bn(c.y.view(M, C, 1, 1))
    rm, rv = R.running_update(rm0, rv0, c.ref)
    assert R.row_err(rm, bn.running_mean) < 1e-10
    assert R.row_err(rv, bn.running_var) < 1e-10
    assert R.row_err(c.ref.unb, c.y.var(0, unbiased=True)) < 1e-10


def test_count_one_keeps_the_biased_variance():
    """M = 1: torch's unbiased variance is undefined; the builders keep var (no division by zero)."""
    t = R.bn_tables(torch.tensor([[0.5, -1.0]]), torch.tensor([[1.25, 3.0]]), None, None, None,
                    torch.ones(2), torch.zeros(2), 1)
    assert torch.equal(t.unb, t.var) and torch.isfinite(t.unb).all()
    assert torch.allclose(t.var, torch.tensor([1.0, 2.0], dtype=torch.float64))


def test_negative_variance_is_clamped():
    t = R.bn_tables(torch.tensor([[4.0]]), torch.tensor([[3.996]]), None, None, None, torch.ones(1), torch.zeros(1), 4)
    assert float(t.var) == 0.0 and abs(float(t.invstd) - R.EPS ** -0.5) < 1e-9


def test_split_replicas_layout():
    gen = torch.Generator().manual_seed(0)
    tot = torch.randn(10, generator=gen, dtype=torch.float64)
    b = R.split_replicas(tot, 5, 18, gen, torch.float64)
    assert b.shape == (5, 18) and torch.isnan(b[:, 10:]).all() and not torch.isnan(b[:, :10]).any()
    assert R.row_err(b[:, :10].sum(0), tot) < 1e-12
    w = b[:, 0] / tot[0]
    assert (w < 0).sum() == 1 and len({round(float(x), 6) for x in w}) == 5
    one = R.split_replicas(tot, 1, 0, gen)
    assert one.shape == (1, 10) and torch.equal(one[0], tot.float())


@pytest.mark.parametrize("C,reps,M", CASES)
def test_fp32_restatement_is_conditioned(C, reps, M):
    """The same function in fp32 from the same fp32 replicas stays within 1e-6 of fp64 on every row
    (relative to the row's max), so the GPU bars (1e-5) are reachable by a correct fp32 builder; and
    every term of the closed-form bias gradient is at least 1e-4 of the three terms' sum on at least
    98 % of the channels, so the GPU bias-gradient bar (1e-6 of that sum) sees a dropped or mis-signed
    term.  (Not on every channel: B·Σy vanishes with the channel mean and with Σg·x̂, which the recipe
    leaves within 1e-4 of zero on about one channel in a thousand; a wrong term is wrong on all.)"""
    c = _case(C, reps, M, torch.float32)
    r = c.rows
    t32 = R.bn_tables(r["sum"], r["sumsq"], r["dgamma"], r["dbeta"], c.shift, c.gamma, c.beta, M, dtype=torch.float32)
    worst = 0.0
    for k in R.FWD_ROWS + R.BWD_ROWS + ("mean", "var", "unb"):
        worst = max(worst, R.row_err(getattr(t32, k), getattr(c.ref, k)))
    for a, b in zip(t32.db_terms, c.ref.db_terms):
        worst = max(worst, R.row_err(a, b))
    print(f"C={C} R={reps} M={M}: fp32 restatement within {worst:.1e} of fp64")
    assert worst < 1e-6
    assert R.db_terms_visible(c.ref) >= 0.98


def test_leaky_relu_and_batch_norm_compose_as_the_table_says():
    c = _case(24, 5, 192, torch.float64)
    want = F.leaky_relu(R.autograd_dy(c)[0], R.SLOPE)
    got = F.leaky_relu(c.ref.a[None] * c.y + c.ref.b[None], R.SLOPE)
    assert R.row_err(got, want) < 1e-10
