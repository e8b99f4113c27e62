"""Which calls the closing-loss kernels take (vae_amd/closers.py: ReconLoss.takes, LogCoshLoss.takes) —
the rules by which the drop-in models choose between the kernel and their torch fallback — and the
closers' own argument checks, without a GPU: the rules read shapes and `is_cuda` only."""
import types

import pytest
import torch

from vae_amd.closers import CLOSERS, LogCoshLoss, ReconLoss

WINDOW = [1 / 11] * 11


def _img(*shape, cuda=True):
    """What the rules read of an image batch on the GPU."""
    return types.SimpleNamespace(is_cuda=cuda, shape=torch.Size(shape), dim=lambda: len(shape))


MSSIM = {"kind": "mssim", "window": WINDOW}


def _center(h, w):
    return {"kind": "center", "mask": torch.ones(h, w, device="meta")}


@pytest.mark.parametrize("cfg,recons,target,takes", [
    (MSSIM, (4, 3, 64, 64), (4, 3, 64, 64), True),
    (MSSIM, (4, 3, 72, 72), (4, 3, 72, 72), False),                 # 72 is no multiple of 2**(5-1)
    (MSSIM, (4, 3, 80, 80), (4, 3, 80, 80), False),                 # a plane of more than 4096
    ({**MSSIM, "levels": 3}, (4, 3, 36, 36), (4, 3, 36, 36), True),     # (its own levels: multiples of 4)
    ({**MSSIM, "levels": 3}, (4, 3, 34, 34), (4, 3, 34, 34), False),
    (_center(64, 64), (4, 3, 64, 64), (4, 3, 64, 64), True),
    (_center(32, 32), (4, 3, 64, 64), (4, 3, 64, 64), False),       # the mask is not the plane's shape
    (_center(64, 64), (4, 3, 64, 64), (4, 3, 32, 32), False),       # unequal planes
    (_center(64, 64), (3, 64, 64), (3, 64, 64), False),             # not 4-D
    (None, (4, 3, 64, 64), (4, 3, 64, 64), False),                  # plain MSE: no recon_loss at all
])
def test_recon_loss_takes(cfg, recons, target, takes):
    assert bool(ReconLoss.takes(cfg, _img(*recons), _img(*target))) is takes
    assert not ReconLoss.takes(cfg, _img(*recons, cuda=False), _img(*target, cuda=False))


@pytest.mark.parametrize("alpha,recons,target,takes", [
    (10.0, (4, 3, 64, 64), (4, 3, 64, 64), True),
    (10.0, (4, 3, 80, 80), (4, 3, 80, 80), True),                   # (streams: no plane limit)
    (10.0, (4, 3, 64, 64), (4, 3, 32, 32), False),
    (10.0, (4, 3, 64, 64), (2, 3, 64, 64), False),
    (10.0, (4, 12288), (4, 12288), False),
    (0.0, (4, 3, 64, 64), (4, 3, 64, 64), False),
    (-1.0, (4, 3, 64, 64), (4, 3, 64, 64), False),
])
def test_logcosh_takes(alpha, recons, target, takes):
    assert bool(LogCoshLoss.takes(alpha, _img(*recons), _img(*target))) is takes
    assert not LogCoshLoss.takes(alpha, _img(*recons, cuda=False), _img(*target, cuda=False))


def test_cpu_tensors_take_the_torch_fallback():
    x = torch.zeros(2, 3, 64, 64)
    assert not ReconLoss.takes(MSSIM, x, x) and not LogCoshLoss.takes(10.0, x, x)


def test_the_closers_check_their_own_arguments():
    from vae_amd.net import StepPlan
    assert CLOSERS == {"logcosh": LogCoshLoss}
    with pytest.raises(ValueError, match="recon_loss kind 'l1'"):
        ReconLoss((4, 3, 64, 64), "cpu", {"kind": "l1"})
    for kw in (dict(samples=2), dict(recon_loss=MSSIM)):
        with pytest.raises(ValueError, match="takes one sample and no recon_loss"):
            StepPlan(None, 8, loss="logcosh", alpha=10.0, **kw)
    with pytest.raises(ValueError, match="needs a finite alpha > 0, got -0.5"):
        StepPlan(None, 8, loss="logcosh")


def test_run_elbo_refuses_every_closing_loss():
    """Before it reads anything of the plan: a loss in CLOSERS has no ELBO kind of its own."""
    from vae_amd.net import StepPlan
    for name, closer in CLOSERS.items():
        assert name in StepPlan.LOSS_KINDS
        with pytest.raises(ValueError, match=closer.fn):
            StepPlan.run_elbo(None, 0, name, 1.0)
