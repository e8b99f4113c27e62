"""The data-parallel LogCoshVAE step: two ranks on one device over gloo (the set-up of
tests/test_gpu_dp_infovae.py), 8 images per rank, fp32.  Each rank's loss is over its own shard, so the
averaged gradient is the mean of the two shards' restatement gradients (tests/logcosh_ref.py) and the
logged terms are the mean of the two shards' terms.  Bars: parity_util.grad_bar, loss terms 1e-4."""
import os

import pytest
import torch
import torch.multiprocessing as mp

from test_gpu_dp import _port

pytestmark = pytest.mark.gpu

B, WORLD, SEED = 8, 2, 1265
YAML = dict(alpha=10.0, beta=1.0)                       # configs/vae/logcosh_vae.yaml
M_N = 0.00025


def _shard(rank):
    from oracle import vae_oracle as O
    return O.make_inputs(B, 128, 300 + rank)


def _worker(rank, port, q):
    try:
        import torch.distributed as dist
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        torch.cuda.set_device(0)
        dist.init_process_group("gloo", rank=rank, world_size=WORLD)
        from oracle import vae_oracle as O
        from vae_amd.engine import FusedAdam, TrainStep
        from vae_amd.net import StepPlan, VAENet
        net = VAENet(latent_dim=128, dtype=torch.float32, device="cuda:0")
        net.load_reference_state_dict(O.make_params(O.vanilla_param_spec(), SEED))
        plan = StepPlan(net, B, loss="logcosh", kld_weight=M_N, **YAML)
        step = TrainStep(net, plan, FusedAdam(net, lr=0.005), graph=True, nbuckets=4)
        assert step.comm is not None and not step.deferred
        x, eps = _shard(rank)
        step(x.cuda(), eps.cuda())
        torch.cuda.synchronize()
        grads = {k: v.cpu().numpy() for k, v in net.layout.export_reference(plan.grads).items()}
        q.put((rank, grads, step.loss_terms(), plan.loss_dict()))
        dist.barrier()
        dist.destroy_process_group()
    except Exception:
        import traceback
        q.put((rank, traceback.format_exc(), None, None))


def test_data_parallel_logcosh_matches_restatement_shard_mean():
    import logcosh_ref as R
    from oracle import vae_oracle as O
    from parity_util import grad_bar
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _port()
    procs = [ctx.Process(target=_worker, args=(r, port, q)) for r in range(WORLD)]
    for p in procs:
        p.start()
    res = {}
    for _ in range(WORLD):
        r, grads, terms, local = q.get(timeout=240)
        assert not isinstance(grads, str), grads
        res[r] = ({k: torch.from_numpy(v) for k, v in grads.items()}, terms, local)
    for p in procs:
        p.join(timeout=60)
    sd = O.make_params(O.vanilla_param_spec(), SEED)
    shards, spreads = zip(*[R.with_spread(sd, *_shard(r), M_N=M_N, **YAML) for r in range(WORLD)])
    spread = {k: max(sp[k] for sp in spreads) for k in spreads[0]}
    for k in res[0][0]:
        assert torch.equal(res[0][0][k], res[1][0][k]), k             # both ranks hold the averaged gradient
    for r in range(WORLD):
        for i, t in enumerate(R.TERMS):
            want = sum(s["loss"][t] for s in shards) / WORLD
            assert abs(res[r][1][i] - want) <= 1e-4 * abs(want), (r, t, res[r][1][i], want)
            own = shards[r]["loss"][t]
            assert abs(res[r][2][t] - own) <= 1e-4 * abs(own), (r, t, res[r][2][t], own)
    gmean = {k: sum(s["grads"][k] for s in shards) / WORLD for k in shards[0]["grads"]}
    worst = 0.0
    for name, gr in gmean.items():
        if R.pre_bn_bias(name):
            continue                                                  # analytically zero under train-mode BN
        err = float((res[0][0][name].double() - gr.double()).norm() / gr.double().norm())
        worst = max(worst, err)
        assert err < grad_bar(name, spread), (name, err, grad_bar(name, spread))
    print(f"DP LogCoshVAE 2x{B}: worst averaged-gradient rel-norm {worst:.2e}")
