"""The LogCoshVAE drop-in model (vae_amd.models.LogCoshVAE; models/logcosh_vae.py:8-176): the BaseVAE
interface on the HIP forward, loss_function with the log-cosh term on the GPU (vae_logcosh_loss through
_HipLogCosh) and the KL in torch, the fused HIP backward seeded by autograd's dL/drecon and
dL/d[mu, log_var]; the torch formula on anything else.  Bars: those of tests/test_gpu_dipvae_model.py."""
import functools
import math

import pytest
import torch

import logcosh_ref as R
from golden_util import load_case

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _case():
    meta, _ = load_case("logcosh_b8")
    sd, x, eps = R.case_inputs(meta)
    ref, spread = R.with_spread(sd, x, eps, M_N=meta["M_N"], **R.loss_kwargs(meta))
    ref["spread"] = spread
    return meta, sd, x, eps, ref


def _model(meta, sd, **ctor):
    from vae_amd.models import vae_models
    m = vae_models["LogCoshVAE"](**{**meta["ctor"], **ctor}, dtype=torch.float32, device="cuda")
    m.load_reference_state_dict(sd)
    return m.train()


def _step(model, meta, x, eps, scale=1.0):
    model.flat.grad = None
    out = model(x.cuda(), eps=eps.cuda())
    ld = model.loss_function(*out, M_N=meta["M_N"])
    (scale * ld["loss"]).backward()
    torch.cuda.synchronize()
    return out, ld, model.flat.grad.clone()


def test_forward_loss_dict_and_backward_match_the_reference():
    meta, sd, x, eps, ref = _case()
    model = _model(meta, sd)
    out, ld, g1 = _step(model, meta, x, eps)
    recons, inp, mu, log_var = out                       # logcosh_vae.py:123
    assert len(out) == 4 and torch.equal(inp.cpu(), x)
    assert recons.shape == x.shape and mu.shape == log_var.shape == (x.shape[0], 128)
    assert tuple(ld) == R.TERMS == ("loss", "Reconstruction_Loss", "KLD")
    assert type(ld["Reconstruction_Loss"].grad_fn).__name__.startswith("_HipLogCosh")
    for k in R.TERMS:
        for want in (ref["loss"][k], meta["loss"][k]):   # the restatement and the reference's own value
            assert abs(float(ld[k].detach()) - want) <= 1e-4 * abs(want), (k, float(ld[k].detach()), want)
    # the gradient is the fused plan's (the same kernels; the seeds go through autograd here): 1e-6
    # relative norm, as for the DIP-VAE drop-in — one fp32 rounding per seed element, carried linearly
    from test_gpu_logcosh_step import _run_plan
    _, runs, _ = _run_plan(sd, x, eps, torch.float32, kld_weight=meta["M_N"], **R.loss_kwargs(meta))
    fused = runs[0][1]
    assert float((g1 - fused).norm() / fused.norm()) <= 1e-6
    # and the restatement's, per tensor
    from parity_util import grad_bar
    grads = {k: v.cpu() for k, v in model.net.layout.export_reference(g1).items()}
    for name, gr in ref["grads"].items():
        if R.pre_bn_bias(name):
            continue
        err = float((grads[name].double() - gr.double()).norm() / gr.double().norm())
        assert err < grad_bar(name, ref["spread"]), (name, err, grad_bar(name, ref["spread"]))
    # loss * 0.37 scales every seed
    _, _, gs = _step(model, meta, x, eps, scale=0.37)
    assert float((gs - 0.37 * g1).norm() / (0.37 * g1).norm()) <= 1e-6


def test_eval_forward_takes_the_torch_formula():
    meta, sd, x, eps, _ = _case()
    kw = R.loss_kwargs(meta)
    model = _model(meta, sd).eval()
    with torch.no_grad():
        out = model(x.cuda(), eps=eps.cuda())
        ld = model.loss_function(*[t.cpu() for t in out], M_N=meta["M_N"])      # CPU tensors: torch formula
        ld_gpu = model.loss_function(*out, M_N=meta["M_N"])
    assert len(out) == 4 and not out[0].requires_grad and ld["loss"].grad_fn is None
    ev = R.train_step(sd, x, eps, M_N=meta["M_N"], training=False, **kw)
    torch.testing.assert_close(out[2].cpu(), ev["mu"], rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(out[3].cpu(), ev["log_var"], rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(out[0].cpu(), ev["recon"], rtol=1e-4, atol=1e-5)
    want = R.logcosh_loss(*[t.cpu() for t in out], meta["M_N"], **kw)
    assert tuple(ld) == tuple(ld_gpu) == R.TERMS
    for k in R.TERMS:
        assert abs(float(ld[k]) - float(want[k])) <= 1e-5 * abs(float(want[k])), (k, float(ld[k]), float(want[k]))
        assert abs(float(ld_gpu[k]) - float(want[k])) <= 1e-5 * abs(float(want[k])), (k, float(ld_gpu[k]))
        assert abs(float(ld[k]) - ev["loss"][k]) <= 1e-4 * abs(ev["loss"][k]), (k, float(ld[k]), ev["loss"][k])


def test_default_constructed_model_is_finite_where_the_reference_overflows():
    """alpha = 100 (the constructor default): the reference's loss is inf on these inputs
    (tests/test_logcosh_ref.py); here it is finite and the fp64 stable form, with a finite gradient."""
    from vae_amd.models import LogCoshVAE
    meta, sd, x, eps, _ = _case()
    model = LogCoshVAE(3, 128, dtype=torch.float32, device="cuda")
    assert (model.alpha, model.beta) == (100., 10.)
    model.load_reference_state_dict(sd)
    model.train()
    out, ld, g = _step(model, meta, x, eps)
    t = out[0].detach().cpu() - x
    assert float(t.min()) < -0.44
    assert math.isinf(float(R.recon_literal(t, 100.0)))
    mulv = torch.cat([out[2].detach().cpu(), out[3].detach().cpu()], 1)
    rl, kld, loss, _ = R.terms64(out[0].detach().cpu(), x, mulv, 100.0, 10.0 * meta["M_N"])
    for k, want in zip(R.TERMS, (loss, rl, -kld)):
        got = float(ld[k].detach())
        assert math.isfinite(got) and abs(got - want) <= 1e-5 * abs(want), (k, got, want)
    assert bool(torch.isfinite(g).all()) and float(g.norm()) > 0


def test_reference_keyed_state_dict_round_trip():
    meta, sd, *_ = _case()
    model = _model(meta, sd)
    got = model.state_dict()
    assert list(got) == list(sd)
    for k, v in sd.items():
        assert torch.equal(got[k].cpu(), v), k
    from vae_amd.models import LogCoshVAE
    other = LogCoshVAE(3, 128, dtype=torch.float32, device="cuda")
    other.load_state_dict({k: v.clone() for k, v in got.items()}, strict=True)
    assert torch.equal(other.flat.detach(), model.flat.detach())
