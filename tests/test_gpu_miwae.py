"""vae_elbo_fwd (VAE_LOSS_MIWAE, csrc/vae_elbo.hpp) alone against the reference's loss
(models/miwae.py:148-164) in fp64 with autograd (tests/miwae_ref.py miwae_elbo64).

The inputs are crafted, because a training step's own cannot tell the groupings apart: kld_b is
constant inside a group and cancels in the softmax, and at initialisation the per-sample MSEs differ
by far less than the bar.  Here sse = img_elems * u with u uniform in [0.05, 3], mulv random with kld_b
in roughly 20..60, M_N = 0.01 — and each case first shows, on the CPU in fp64, that the two wrong
groupings a kernel could implement (one softmax over all M*K rows; k-major groups) give coefficients
more than 100 bars away from the right one's (k-major at K = 1 is the right grouping and is left out).

Bars (the project's op bars): out[0..3] within 1e-4 relative, per_img / head_coef / kl_coef within 1e-4
relative norm (measured on one MI355X: worst 1.7e-7, head_coef / kl_coef; out 9.8e-8).  Shapes: (B, M, K) = (4,3,5) the yaml's, (7,2,3), (1,5,5) the defaults at one image,
(3,4,1) K = 1, (300,3,5) more groups than threads, (1024,2,1) the kld_row limit."""
import ctypes
import functools

import pytest
import torch

import miwae_ref as R

pytestmark = pytest.mark.gpu

IMG, D, M_N, BAR = 3 * 64 * 64, 32, 0.01, 1e-4
SHAPES = [(4, 3, 5), (7, 2, 3), (1, 5, 5), (3, 4, 1), (300, 3, 5), (1024, 2, 1)]


@functools.lru_cache(maxsize=None)
def _inputs(B, S, seed=0):
    """(sse [B*S], mulv [B, 2D]): sse = img * U[0.05, 3]; mu ~ N(0, 1.3), log_var ~ 0.5 N: kld_b 20..60."""
    g = torch.Generator().manual_seed(7919 * B + 31 * S + seed)
    sse = IMG * (0.05 + 2.95 * torch.rand(B * S, generator=g))
    mulv = torch.cat([1.3 * torch.randn(B, D, generator=g), 0.5 * torch.randn(B, D, generator=g)], 1)
    return sse, mulv


def run_elbo(kind, sse, mulv, samples, estimates):
    """One vae_elbo_fwd: (out, per_img, head_coef, kl_coef) on the CPU; the outputs start NaN-filled."""
    from vae_amd import _lib as L
    B = mulv.shape[0]
    f = dict(dtype=torch.float32, device="cuda")
    sse_d, mulv_d = sse.to(**f).contiguous(), mulv.to(**f).contiguous()
    out, per, hc, kc = (torch.full((n,), float("nan"), **f) for n in (4, B * samples, B * samples, B * samples))
    e = L.ElboArgs(kind=kind, batch=B, samples=samples, latent=mulv.shape[1] // 2, img_elems=IMG, kld_weight=M_N,
                   mmd_tiles=estimates)
    e.mulv, e.sse, e.out, e.per_img, e.head_coef, e.kl_coef = (t.data_ptr() for t in (mulv_d, sse_d, out, per, hc, kc))
    L.call("vae_elbo_fwd", ctypes.byref(e), L.stream_ptr())
    torch.cuda.synchronize()
    return out.cpu(), per.cpu(), hc.cpu(), kc.cpu()


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


@pytest.mark.parametrize("B,M,K", SHAPES)
def test_miwae_elbo_matches_fp64(B, M, K):
    from vae_amd import _lib as L
    sse, mulv = _inputs(B, M * K)
    kld = R.kld_rows(mulv.double())
    assert 10.0 < float(kld.min()) and float(kld.max()) < 90.0, (float(kld.min()), float(kld.max()))
    want = R.miwae_elbo64(sse, mulv, M, K, M_N, IMG)
    # The wrong groupings are far outside the bars, so passing them means the grouping is right: the
    # coefficients by more than 100 bars (0.37 rel-norm at the least on these inputs).  The loss is a
    # mean over the B*M groups in which the groups' differences partly cancel (1.6e-3 at (300,3,5),
    # k-major): it is asserted at 10 bars and printed.  'all' equals the right grouping at M = 1,
    # 'kmajor' at M = 1 or K = 1.
    for wrong in ("all", "kmajor"):
        if M == 1 or (wrong == "kmajor" and K == 1):
            continue
        w = R.miwae_elbo64(sse, mulv, M, K, M_N, IMG, grouping=wrong)
        dl = abs(float(w[0][0] - want[0][0])) / abs(float(want[0][0]))
        dh, dk = _rel(w[2], want[2]), _rel(w[3], want[3])
        print(f"({B},{M},{K}) grouping {wrong}: loss off by {dl:.2e}, head_coef by {dh:.2e}, kl_coef by {dk:.2e}")
        assert dh > 100 * BAR and dk > 100 * BAR and dl > 10 * BAR, (wrong, dl, dh, dk)
    got = run_elbo(L.LOSS_MIWAE, sse, mulv, M * K, M)
    errs = [abs(float(got[0][i] - want[0][i])) / abs(float(want[0][i])) for i in range(4)]
    errs += [_rel(got[i], want[i]) for i in (1, 2, 3)]
    print(f"({B},{M},{K}): out rel err {errs[:4]}, per_img / head_coef / kl_coef rel-norm {errs[4:]}")
    assert max(errs) <= BAR, errs
    # ordered reductions: a second call gives the same bits
    again = run_elbo(L.LOSS_MIWAE, sse, mulv, M * K, M)
    for a, b in zip(got, again):
        assert torch.equal(a, b)
    if K == 1:
        # one sample per group: w = 1, g = 1/(B*M) for every row
        uni = 2.0 / (B * M * IMG)
        assert float((got[2] - uni).abs().max()) <= 1e-6 * uni, (float(got[2].min()), float(got[2].max()), uni)


@pytest.mark.parametrize("B,S", [(4, 5), (7, 15), (300, 5), (64, 15), (3, 12)])
def test_one_estimate_is_iwae_bit_for_bit(B, S):
    """IWAE is the one-group case of the same branch: kind IWAE with S samples and kind MIWAE with
    M = 1, samples = S give the same out, per_img, head_coef and kl_coef (S = 5 and 15; 12 takes the
    path that recomputes in place of the registers)."""
    from vae_amd import _lib as L
    sse, mulv = _inputs(B, S, seed=5)
    iw = run_elbo(L.LOSS_IWAE, sse, mulv, S, 0)
    mi = run_elbo(L.LOSS_MIWAE, sse, mulv, S, 1)
    for a, b in zip(iw, mi):
        assert torch.equal(a, b)
    want = R.miwae_elbo64(sse, mulv, 1, S, M_N, IMG)
    assert abs(float(iw[0][0] - want[0][0])) <= BAR * abs(float(want[0][0]))
    assert _rel(iw[2], want[2]) <= BAR and _rel(iw[3], want[3]) <= BAR


@pytest.mark.parametrize("B,M,K", [(5, 2, 12), (260, 1, 9)])
def test_large_k_recompute_path_matches_fp64(B, M, K):
    """K above the register path's 8 samples a group."""
    from vae_amd import _lib as L
    sse, mulv = _inputs(B, M * K, seed=9)
    want = R.miwae_elbo64(sse, mulv, M, K, M_N, IMG)
    got = run_elbo(L.LOSS_MIWAE, sse, mulv, M * K, M)
    errs = [abs(float(got[0][i] - want[0][i])) / abs(float(want[0][i])) for i in range(4)]
    errs += [_rel(got[i], want[i]) for i in (1, 2, 3)]
    print(f"({B},{M},{K}): {errs}")
    assert max(errs) <= BAR, errs
