"""vae_logcosh_loss (csrc/vae_logcosh.hip) alone against the fp64 stable form on the same fp32 inputs
(tests/logcosh_ref.terms64): the log-cosh term, its tanh seed, the KL term with its coefficient, the
loss dict and the per-image MSE.

Bars: those of tests/test_gpu_recon_loss.py — the loss within 1e-5 relative + 1e-7, the seed's
relative norm below 1e-5 — and 1e-5 relative for the KL terms (stepcheck's teacher-forced bar).
Shapes: the smallest batch, the project's odd last-batch sizes, and 35 elements per image (3 x 35 =
105 values: 26 vector groups and a one-element tail; with a 4-byte offset, every element one at a time)."""
import ctypes

import numpy as np
import pytest
import torch

import logcosh_ref as R

pytestmark = pytest.mark.gpu

SHAPES = [(1, 3, 64, 64), (7, 3, 64, 64), (19, 3, 16, 16), (3, 1, 5, 7)]
CRAFTED = (0.0, 1e-4, -1e-4, 0.44, -0.44, 1.99, -1.99)


def _inputs(shape, seed):
    """recon in (-1, 1), target in [-1, 1], seeded; the first elements of every image crafted so that
    t = recon - target takes each value of CRAFTED (as closely as fp32 allows)."""
    g = torch.Generator().manual_seed(seed)
    target = 2 * torch.rand(shape, generator=g) - 1
    recon = (2 * torch.rand(shape, generator=g) - 1) * 0.999
    r, t = recon.view(shape[0], -1), target.view(shape[0], -1)
    for i, v in enumerate(CRAFTED):
        t[:, i] = -0.5 * v
        r[:, i] = 0.5 * v
    return recon, target


def _call(recon, target, alpha, mulv=None, kl_weight=0.0, sse=None, grad=True, offset=0, repeats=1):
    """vae_logcosh_loss on the device; outputs start NaN-filled.  offset: elements by which recon,
    target and grad are shifted inside their allocations (4-byte steps off the 16-byte alignment)."""
    from vae_amd import _lib as L
    n, elems = recon.shape[0], recon[0].numel()
    dev = "cuda"

    def place(t):
        buf = torch.zeros(t.numel() + offset, device=dev)
        buf[offset:].copy_(t.flatten())
        return buf

    rb, tb = place(recon), place(target)
    a = L.logcosh_args(n, elems, alpha, kl_weight=kl_weight, latent=0 if mulv is None else mulv.shape[1] // 2)
    a.recon, a.target = rb.data_ptr() + 4 * offset, tb.data_ptr() + 4 * offset
    gb = torch.full((n * elems + offset,), float("nan"), device=dev)
    if grad:
        a.grad = gb.data_ptr() + 4 * offset
    out = torch.full((4,), float("nan"), device=dev)
    a.out = out.data_ptr()
    klc = torch.full((n + 3,), float("nan"), device=dev)
    if mulv is not None:
        mv = mulv.cuda().contiguous()
        a.mulv, a.kl_coef = mv.data_ptr(), klc.data_ptr()
    per = torch.full((n + 3,), float("nan"), device=dev)
    if sse is not None:
        sb = sse.cuda()
        a.sse, a.per_img = sb.data_ptr(), per.data_ptr()
    ws = torch.zeros(L.logcosh_workspace(a) // 8, dtype=torch.float64, device=dev)
    a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel() * 8
    runs = []
    for _ in range(repeats):
        L.call("vae_logcosh_loss", ctypes.byref(a), L.stream_ptr())
        torch.cuda.synchronize()
        runs.append(dict(out=out.cpu(), grad=gb[offset:].cpu().view(recon.shape), kl_coef=klc.cpu(), per_img=per.cpu(),
                         pad=gb[:offset].cpu()))
    return runs if repeats > 1 else runs[0]


@pytest.mark.parametrize("alpha", [10.0, 100.0])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_loss_and_seed_match_fp64(shape, alpha):
    recon, target = _inputs(shape, 11 + shape[0])
    tv = (recon - target).view(shape[0], -1)[0, :len(CRAFTED)]
    np.testing.assert_allclose(tv.numpy(), CRAFTED, rtol=1e-6, atol=0)
    rl, _, _, seed = R.terms64(recon, target, None, alpha, 0.0)
    got = _call(recon, target, alpha)
    o = got["out"].tolist()
    print(f"{shape} alpha {alpha}: hip {o[1]:.9g} fp64 {rl:.12g} rel {abs(o[1] - rl) / rl:.2e}; seed rel-norm "
          f"{float((got['grad'].double() - seed).norm() / seed.norm()):.2e}")
    assert all(np.isfinite(o)) and bool(torch.isfinite(got["grad"]).all())
    assert abs(o[1] - rl) <= 1e-5 * abs(rl) + 1e-7, (o, rl)
    assert o[0] == o[1] and o[2] == 0.0 and o[3] == 0.0             # without mulv
    assert float((got["grad"].double() - seed).norm() / seed.norm()) < 1e-5
    assert bool(torch.isnan(got["kl_coef"]).all()) and bool(torch.isnan(got["per_img"]).all())     # not touched
    # the seed has the sign of t and is exactly 0 where t is
    t = recon - target
    assert bool((got["grad"][t == 0] == 0).all()) and bool((got["grad"] * t >= 0).all())


@pytest.mark.parametrize("latent", [32, 128])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kl_terms_coefficient_and_per_image_mse(shape, latent):
    n = shape[0]
    recon, target = _inputs(shape, 23 + n)
    g = torch.Generator().manual_seed(latent + n)
    mu = torch.randn(n, latent, generator=g)
    lv = 9 * torch.rand(n, latent, generator=g) - 6                 # log_var in [-6, 3]
    mulv = torch.cat([mu, lv], 1)
    sse = torch.rand(n, generator=g) * 1000
    alpha, klw = 10.0, 10.0 * 0.00025
    rl, kld, loss, _ = R.terms64(recon, target, mulv, alpha, klw)
    got = _call(recon, target, alpha, mulv=mulv, kl_weight=klw, sse=sse, grad=False)
    o = got["out"].numpy()
    print(f"{shape} D={latent}: kld hip {o[3]:.9g} fp64 {kld:.12g} rel {abs(o[3] - kld) / abs(kld):.2e}")
    assert abs(o[1] - rl) <= 1e-5 * abs(rl) + 1e-7
    assert abs(o[3] - kld) <= 1e-5 * abs(kld) and abs(o[2] + kld) <= 1e-5 * abs(kld) and o[2] == -o[3]
    assert abs(o[0] - loss) <= 1e-5 * abs(loss) + 1e-7
    # loss = Reconstruction_Loss + kl_weight * kld in fp32, to one ulp (the product may be fused)
    want = np.float32(o[1]) + np.float32(klw) * np.float32(o[3])
    assert abs(np.float32(o[0]) - want) <= np.spacing(np.float32(abs(want))), (o, want)
    klc = got["kl_coef"].numpy()
    assert (klc[:n] == np.float32(klw) / np.float32(n)).all() and np.isnan(klc[n:]).all()
    per = got["per_img"].numpy()
    np.testing.assert_allclose(per[:n], sse.numpy() / np.float32(recon[0].numel()), rtol=2e-7, atol=0)
    assert np.isnan(per[n:]).all()
    assert bool(torch.isnan(got["grad"]).all())                     # grad NULL: nothing written


def test_repeated_calls_are_bit_identical():
    recon, target = _inputs((19, 3, 16, 16), 5)
    g = torch.Generator().manual_seed(2)
    mulv = torch.cat([torch.randn(19, 32, generator=g), 9 * torch.rand(19, 32, generator=g) - 6], 1)
    a, b = _call(recon, target, 100.0, mulv=mulv, kl_weight=0.0025, sse=torch.ones(19), repeats=2)
    for k in ("out", "grad", "kl_coef", "per_img"):
        assert torch.equal(a[k].nan_to_num(7.0), b[k].nan_to_num(7.0)), k
    assert bool(torch.isfinite(a["out"]).all()) and bool(torch.isfinite(a["grad"]).all())


@pytest.mark.parametrize("offset", [1, 2, 3])
def test_unaligned_rows_take_the_scalar_path(offset):
    """recon / target / grad off the 16-byte alignment: the same values as the aligned call to rounding,
    nothing written in front of the first element."""
    shape = (3, 1, 5, 7)
    recon, target = _inputs(shape, 9)
    base = _call(recon, target, 10.0)
    got = _call(recon, target, 10.0, offset=offset)
    rl, _, _, seed = R.terms64(recon, target, None, 10.0, 0.0)
    assert abs(float(got["out"][1]) - rl) <= 1e-5 * abs(rl) + 1e-7
    assert float((got["grad"].double() - seed).norm() / seed.norm()) < 1e-5
    # the same per-element arithmetic on both paths, up to where the compiler fuses a multiply-add
    torch.testing.assert_close(got["grad"], base["grad"], rtol=3e-7, atol=0)
    assert bool(torch.isnan(got["pad"]).all())
