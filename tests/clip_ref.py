"""The reference of the gradient-clipping tests: torch.nn.utils.clip_grad_norm_ +
torch.optim.Adam on the CPU over a flat parameter and given fp32 gradients (Lightning 1.5.6's
gradient_clip_val), in fp64 by default."""
import torch

# the bars of test_gpu_adam.py, held against fp64 here:
BARS = (2e-6, 1e-6, 1e-6)           # parameters (absolute), exp_avg and exp_avg_sq (of the maximum)


def trajectory(p0, grads, max_norm, wd=0.0, lr=5e-3, betas=(0.9, 0.999), dtype=torch.float64):
    """Per step (parameters, exp_avg, exp_avg_sq, norm, coef) from the fp32 start p0."""
    ref = p0.detach().cpu().to(dtype).clone().requires_grad_(True)
    opt = torch.optim.Adam([ref], lr=lr, betas=betas, eps=1e-8, weight_decay=wd)
    out = []
    for gk in grads:
        ref.grad = gk.detach().cpu().to(dtype).clone()
        norm = float(torch.nn.utils.clip_grad_norm_([ref], max_norm))
        opt.step()
        st = opt.state[ref]
        out.append((ref.detach().clone(), st["exp_avg"].clone(), st["exp_avg_sq"].clone(), norm,
                    min(1.0, max_norm / (norm + 1e-6))))
    return out
