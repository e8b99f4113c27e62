"""FusedAdam(max_grad_norm=...) — vae_grad_sumsq + vae_adam_step_clip — against
torch.nn.utils.clip_grad_norm_ + torch.optim.Adam in fp64 on the CPU (Lightning 1.5.6's
trainer_params.gradient_clip_val: the clip sits between backward and optimizer.step).

Adam's first step is invariant to the scale of g (m̂ / sqrt(v̂) = sign(g)), so the parameters after
one step cannot see the clip; the moment buffers can, and so can steps 2-5.  Both are compared after
every step."""
import functools
import types

import pytest
import torch

import clip_ref as R

pytestmark = pytest.mark.gpu

N, MAX_NORM, LR, BETAS = 200_003, 0.8, 5e-3, (0.9, 0.999)
SCALES = (1.0, 0.1, 3.0, 1e-3, 0.5)          # gradient norms ~ 447, 45, 1342, 0.45, 224: step 4 is not clipped


@functools.lru_cache(maxsize=None)
def _inputs(n=N, seed=7, scales=SCALES):
    g = torch.Generator().manual_seed(seed)
    p0 = torch.randn(n, generator=g)
    return p0, tuple(torch.randn(n, generator=g) * s for s in scales)


@functools.lru_cache(maxsize=None)
def _reference(wd, max_norm=MAX_NORM, n=N, seed=7, scales=SCALES):
    """The fp64 trajectory of clip_ref on the inputs of _inputs: computed once, shared, left unchanged."""
    p0, grads = _inputs(n, seed, scales)
    return R.trajectory(p0, grads, max_norm, wd=wd, lr=LR, betas=BETAS)


def _net(p0, lowp=True):
    n = p0.numel()
    return types.SimpleNamespace(params=p0.cuda(), device=torch.device("cuda"), swap_descs=[],
                                 lowp=torch.zeros(n, dtype=torch.bfloat16, device="cuda") if lowp else None)


def _step(fa, g):
    from vae_amd import _lib as L
    L.call("vae_step_begin", None, 0, fa.step.data_ptr(), L.stream_ptr())      # ++step (as every training step)
    fa.apply(g)


def _check(fa, net, want, k, bars=R.BARS):
    p, m, v, norm, coef = want
    got = net.params.cpu()
    print(f"step {k}: |dp| {float((got.double() - p).abs().max()):.3e}  "
          f"|dm|/max {float((fa.m.cpu().double() - m).abs().max() / m.abs().max()):.3e}  "
          f"|dv|/max {float((fa.v.cpu().double() - v).abs().max() / v.abs().max()):.3e}  "
          f"norm {float(fa.grad_norm[0]):.9g} vs {norm:.12g}  coef {float(fa.grad_norm[1]):.9g} vs {coef:.12g}")
    assert float((got.double() - p).abs().max()) <= bars[0], (k, bars)
    assert float((fa.m.cpu().double() - m).abs().max()) <= bars[1] * float(m.abs().max()), (k, bars)
    assert float((fa.v.cpu().double() - v).abs().max()) <= bars[2] * float(v.abs().max()), (k, bars)
    if net.lowp is not None:
        assert torch.equal(net.lowp.cpu(), got.to(torch.bfloat16)), k
    # the squares are exact in double and the double sum is good to n * 2^-53: the only rounding that
    # shows is the final conversion to fp32
    gn, gc = (float(t) for t in fa.grad_norm.cpu())
    assert abs(gn - norm) <= 2.0 ** -23 * norm, (k, gn, norm)
    # coef = fp32(fp32(max_norm) / fp32(norm + 1e-6)): four roundings of 2^-24 each; twice that allowed
    assert abs(gc - coef) <= 4 * 2.0 ** -23 * coef, (k, gc, coef)


@pytest.mark.parametrize("wd", [0.0, 0.05])
def test_clipped_adam_matches_fp64_clip_grad_norm_and_adam(wd):
    """Five steps at n = 200 003 (not a multiple of 4: the tail) on gradients of norm ~447, 45, 1342,
    0.45 and 224 with max_norm = 0.8: every step but the fourth is clipped.  Bars: those of
    test_gpu_adam.py, held against fp64 (clip_ref.BARS: 2e-6 absolute on the parameters, 1e-6 of the
    buffer's maximum on both moments), the bf16 copy the rounded parameters.  Measured on an MI355X,
    worst step: 7.4e-7, 1.3e-7, 2.8e-7 (weight decay 0) and 6.7e-7, 9.8e-8, 2.1e-7 (0.05).  For scale,
    torch's own fp32 CPU clip_grad_norm_ + Adam on these inputs is 7.4e-7, 1.5e-6, 3.0e-6 and 1.1e-5,
    2.0e-6, 1.7e-7 from the same reference: it takes the norm in fp32."""
    from vae_amd.engine import FusedAdam
    p0, grads = _inputs()
    want = _reference(wd)
    net = _net(p0)
    fa = FusedAdam(net, lr=LR, betas=BETAS, eps=1e-8, weight_decay=wd, max_grad_norm=MAX_NORM)
    for k, gk in enumerate(grads):
        g = gk.cuda()
        _step(fa, g)
        torch.cuda.synchronize()
        assert int(fa.step.item()) == k + 1
        _check(fa, net, want[k], k)
        clipped = float(fa.grad_norm[1]) < 1.0
        assert clipped == (k != 3), (k, fa.grad_norm)
        if not clipped:
            assert float(fa.grad_norm[1]) == 1.0
        assert torch.equal(g.cpu(), gk), k                     # the gradient buffer stays unclipped
    assert float((net.params.cpu() - p0).abs().max()) > 3 * LR   # (the trajectory moved well beyond rounding)


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("n", [1, 3, 5, 1027])
def test_small_sizes_and_the_scalar_route(n, offset):
    """Fewer elements than one quad, a tail behind one quad, more than one workgroup of quads with a
    tail; offset 1: the gradient starts one element past a 16-byte boundary, so both launches take
    their one-element-per-access route."""
    from vae_amd.engine import FusedAdam
    scales = (1.0, 0.05, 2.0)
    p0, grads = _inputs(n, 11 + n, scales)
    want = _reference(0.05, 0.1, n, 11 + n, scales)
    net = _net(p0)
    fa = FusedAdam(net, lr=LR, betas=BETAS, eps=1e-8, weight_decay=0.05, max_grad_norm=0.1)
    buf = torch.zeros(n + 8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    g = buf[offset:offset + n]
    for k, gk in enumerate(grads):
        buf.fill_(float("nan"))                                # (a read past either end would show)
        g.copy_(gk)
        _step(fa, g)
        torch.cuda.synchronize()
        _check(fa, net, want[k], k)


def test_zero_gradient_leaves_the_parameters_alone():
    from vae_amd.engine import FusedAdam
    p0, _ = _inputs(1027, 3, (1.0,))
    net = _net(p0)
    fa = FusedAdam(net, lr=LR, max_grad_norm=MAX_NORM)
    _step(fa, torch.zeros(1027, device="cuda"))
    torch.cuda.synchronize()
    assert fa.grad_norm.tolist() == [0.0, 1.0]
    assert torch.equal(net.params.cpu(), p0)
    assert not fa.m.any() and not fa.v.any()


def test_a_huge_threshold_is_bitwise_vae_adam_step():
    """coef is exactly 1, and g * 1 is g: parameters, both moments and the bf16 copy equal the
    unclipped launch's bit for bit."""
    from vae_amd.engine import FusedAdam
    p0, grads = _inputs()
    nets = [_net(p0), _net(p0)]
    fas = [FusedAdam(nets[0], lr=LR, weight_decay=0.05), FusedAdam(nets[1], lr=LR, weight_decay=0.05, max_grad_norm=1e30)]
    for k, gk in enumerate(grads):
        g = gk.cuda()
        for fa in fas:
            _step(fa, g)
        torch.cuda.synchronize()
        assert float(fas[1].grad_norm[1]) == 1.0
        assert torch.equal(nets[0].params, nets[1].params), k
        assert torch.equal(fas[0].m, fas[1].m) and torch.equal(fas[0].v, fas[1].v), k
        assert torch.equal(nets[0].lowp, nets[1].lowp), k


def test_two_runs_are_bit_identical_and_the_threshold_is_a_device_scalar():
    from vae_amd.engine import FusedAdam
    p0, grads = _inputs()
    runs = []
    for _ in range(2):
        net = _net(p0, lowp=False)
        fa = FusedAdam(net, lr=LR, max_grad_norm=MAX_NORM)
        norms = []
        for gk in grads[:3]:
            _step(fa, gk.cuda())
            norms.append(fa.grad_norm.clone())
        runs.append((torch.stack(norms).cpu(), net.params.cpu(), fa))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    fa = runs[1][2]
    fa.set_max_grad_norm(1e30)
    _step(fa, grads[0].cuda())
    assert float(fa.grad_norm[1]) == 1.0
    with pytest.raises(ValueError):
        fa.set_max_grad_norm(0.0)
    with pytest.raises(ValueError):
        FusedAdam(_net(p0[:8]), lr=LR, max_grad_norm=-1.0)
    with pytest.raises(RuntimeError, match="defer"):
        fa.apply_deferred(grads[0].cuda(), [], None)
