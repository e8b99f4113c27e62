"""Gradient-norm clipping (the reference trainer's gradient_clip_val) at every public layer, without
a GPU: the runner's flag, the keyword on fit / GraphedSteps / fused_train_step / FusedAdam, and the
two C-ABI entry points (include/vaehip.h vae_grad_sumsq, vae_adam_step_clip)."""
import ctypes
import inspect
import os
import re

import pytest

from vae_amd import _lib as L

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "vaehip.h")


def test_the_runner_has_the_opt_in_flag():
    from vae_amd.run import build_parser
    p = build_parser()
    assert p.parse_args([]).clip_gradients is False
    assert p.parse_args(["--clip_gradients"]).clip_gradients is True


def test_fit_and_graphed_steps_take_gradient_clip_val():
    from vae_amd import experiment
    for fn in (experiment.fit, experiment.GraphedSteps.__init__):
        par = inspect.signature(fn).parameters
        assert "gradient_clip_val" in par and par["gradient_clip_val"].default is None, fn


@pytest.mark.parametrize("cls", ["VanillaVAE", "BetaVAE", "InfoVAE", "Autoencoder", "VQVAE"])
def test_every_fused_train_step_takes_max_grad_norm(cls):
    from vae_amd import models
    par = inspect.signature(getattr(models, cls).fused_train_step).parameters
    if "max_grad_norm" not in par:             # (BetaVAE forwards *args, **kwargs to _HipVAE's)
        assert any(q.kind is q.VAR_KEYWORD for q in par.values()), cls
        par = inspect.signature(models._HipVAE.fused_train_step).parameters
    assert par["max_grad_norm"].default is None, cls


def test_fused_adam_and_train_step_signatures():
    from vae_amd.engine import FusedAdam
    par = inspect.signature(FusedAdam.__init__).parameters
    assert par["max_grad_norm"].default is None
    assert callable(FusedAdam.set_max_grad_norm)


def test_the_header_declares_and_the_binding_lists_both_entry_points():
    src = open(HEADER).read()
    for name in ("vae_grad_sumsq", "vae_adam_step_clip"):
        assert re.search(r"^int %s\(" % name, src, flags=re.M), name
        assert name in L.EXPORTED, name
    m = re.search(r"#define VAE_SUMSQ_MAX_PARTS (\d+)", src)
    assert m and int(m.group(1)) == L.SUMSQ_MAX_PARTS == 1024
    # vae_adam_step's arguments, then partials, nparts, max_norm, norm_out, stream
    assert L._SIGS["vae_adam_step_clip"][:12] == L._SIGS["vae_adam_step"][:12]
    assert len(L._SIGS["vae_adam_step_clip"]) == len(L._SIGS["vae_adam_step"]) + 4


def test_bad_arguments_fail_before_any_launch():
    lib = L.load()
    n = ctypes.c_int32(7)
    assert lib.vae_grad_sumsq(16, None, None, ctypes.byref(n), None) == -1 and n.value == 0
    assert b"grad_sumsq" in lib.vae_last_error()
    assert lib.vae_grad_sumsq(0, None, None, ctypes.byref(n), None) == 0 and n.value == 0
    fake = 1 << 20
    args = [16, fake, fake, fake, fake, fake, fake, 0.9, 0.999, 1e-8, 0.0, None, fake]
    for nparts in (0, L.SUMSQ_MAX_PARTS + 1):
        assert lib.vae_adam_step_clip(*args, nparts, fake, fake, None) == -1
        assert b"partials" in lib.vae_last_error()
    assert lib.vae_adam_step_clip(*args, 1, None, fake, None) == -1
    assert b"adam_step_clip: null" in lib.vae_last_error()
