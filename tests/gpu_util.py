"""Helpers for the GPU tests: NHWC/NCHW moves and BatchNorm transform descriptors built
from torch tensors, so single C-ABI entry points can be checked against PyTorch-CPU fp32."""
import torch

from vae_amd import _lib as L


def nhwc(t_nchw, dtype):
    return t_nchw.permute(0, 2, 3, 1).contiguous().to(device="cuda", dtype=dtype)


def to_nchw(t_nhwc):
    return t_nhwc.float().permute(0, 3, 1, 2).contiguous().cpu()


class BNState:
    """A pre-BN NHWC tensor y plus BN params and the producer-side sums the kernels read."""

    def __init__(self, y_nchw, shift=None, seed=0, dtype=torch.float32, reps=1, rstride=None):
        """reps > 1: the sums (and the dgamma / dbeta handed to xf()) are spread over `reps` unequal
        replica rows `rstride` floats apart (default C) with NaN between them, as bn_ref.split_replicas
        makes them; the totals stay in .sum / .sumsq."""
        g = torch.Generator().manual_seed(seed)
        C = y_nchw.shape[1]
        self.y_nchw = y_nchw
        self.gamma = 0.8 + 0.4 * torch.rand(C, generator=g)
        self.beta = (torch.rand(C, generator=g) * 2 - 1) * 0.1
        self.shift = shift if shift is not None else torch.zeros(C)
        d = (y_nchw - self.shift.view(1, -1, 1, 1)).double()
        self.sum = d.sum(dim=(0, 2, 3)).float()
        self.sumsq = (d * d).sum(dim=(0, 2, 3)).float()
        self.count = y_nchw.numel() // C
        self.dev = {k: getattr(self, k).cuda() for k in ("gamma", "beta", "shift", "sum", "sumsq")}
        self.reps, self.rstride = reps, (C if rstride is None else rstride)
        self._gen, self._keep = torch.Generator().manual_seed(seed + 1), []
        if reps > 1:
            for k in ("sum", "sumsq"):
                self.dev[k] = self.replicated(getattr(self, k))
        self.y_dev = nhwc(y_nchw, dtype)

    def replicated(self, total):
        """A [C] total as this state's replica rows on the device."""
        from bn_ref import split_replicas
        return split_replicas(total.detach().cpu(), self.reps, self.rstride, self._gen).contiguous().cuda()

    def act_ref(self):
        """lrelu(BN_train(y)) in PyTorch, NCHW fp32 CPU."""
        yb = torch.nn.functional.batch_norm(self.y_nchw, None, None, self.gamma, self.beta, True, 0.1, 1e-5)
        return torch.nn.functional.leaky_relu(yb, 0.01)

    def xf(self, kind=L.X_BN_ACT, aux=None, dgamma=None, dbeta=None):
        C = self.gamma.numel()
        x = L.Xform(kind=kind, channels=C, slope=0.01, count=float(self.count), eps=1e-5, momentum=0.1)
        x.sum = self.dev["sum"].data_ptr()
        x.sumsq = self.dev["sumsq"].data_ptr()
        x.shift = self.dev["shift"].data_ptr()
        x.gamma = self.dev["gamma"].data_ptr()
        x.beta = self.dev["beta"].data_ptr()
        if self.reps > 1:
            x.reps, x.rstride = self.reps, self.rstride
        if kind in (L.X_BN_DY,):
            if self.reps > 1:
                dgamma, dbeta = self.replicated(dgamma), self.replicated(dbeta)
                self._keep += [dgamma, dbeta]
            x.dgamma = dgamma.data_ptr()
            x.dbeta = dbeta.data_ptr()
        if aux is not None:
            x.aux = aux.data_ptr()
        return x


def rel(a, b):
    a = a.double().flatten()
    b = b.double().flatten()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def tol(dtype):
    return 2e-5 if dtype == torch.float32 else 2e-2


def vq_argmin_clear(z, E):
    """fp64 nearest code of every row of z [rows, dim] in the codebook E [codes, dim] by the
    reference's formula (Σz² + ΣE²) − 2 z·E (vq_vae.py:30-32), and the rows whose winner an fp32
    evaluation of that formula cannot change.  Returns (argmin, clear mask).

    A row is clear when its top-2 distance gap exceeds 2·(2·dim + 4)·2⁻²⁴·(|z|² + max_k|E_k|²):
    Σz², ΣE² and z·E are fma chains of length dim, so each carries at most dim·u relative to its
    sum of magnitudes (u = 2⁻²⁴, fp32 round-to-nearest), and |2 z·E| ≤ |z|² + |E_k|²; the add of
    the two norms, the doubling and the final subtraction add at most 4u of the same scale.  One
    distance is therefore off by at most (2·dim + 4)·u·(|z|² + |E_k|²), and two distances can
    swap order only inside twice that."""
    z, E = z.double(), E.double()
    zz, ee = (z * z).sum(1), (E * E).sum(1)
    dist = zz[:, None] + ee[None, :] - 2.0 * (z @ E.t())
    want = torch.argmin(dist, dim=1)
    top2 = torch.topk(dist, 2, dim=1, largest=False).values
    bar = 2.0 * (2 * z.shape[1] + 4) * 2.0 ** -24 * (zz + ee.max())
    return want, (top2[:, 1] - top2[:, 0]) > bar


def check_vq_indices(latpre, E, indices, tag, slope=0.01):
    """A VQ step's code indices against the fp64 argmin over the latents the quantizer itself read:
    lrelu(latpre) of the step's stored pre-activation latents [..., dim] (device, the step's dtype)
    and the fp32 codebook E [codes, dim] the step ran with.  Exact on every clear row
    (vq_argmin_clear), and at least 95 % of the rows must be clear."""
    pre = latpre.detach().float().cpu().reshape(-1, E.shape[1])
    want, clear = vq_argmin_clear(torch.nn.functional.leaky_relu(pre, slope), E.detach().float().cpu())
    idx = indices.cpu()
    assert idx.numel() == pre.shape[0]
    n_clear = int(clear.sum())
    mism = int((idx[clear] != want[clear]).sum())
    print(f"{tag}: {n_clear} of {idx.numel()} rows clear ({100.0 * n_clear / idx.numel():.2f} %), "
          f"{mism} clear rows differ from the fp64 argmin, {int((idx != want).sum())} rows differ in total")
    assert n_clear >= 0.95 * idx.numel(), (n_clear, idx.numel())
    assert mism == 0, mism


def give_workspace(a, *fns):
    """Query the workspace the calls `fns` need for args `a` (vae_*_workspace_size), allocate
    it and point `a` at it; returns the buffer (keep it alive until the calls are done)."""
    need = max(L.workspace_size(fn, a) for fn in fns)
    ws = torch.empty(max(1, (need + 3) // 4), device="cuda")
    a.workspace = ws.data_ptr()
    a.workspace_bytes = ws.numel() * 4
    return ws


def launched(fn):
    """Run fn() with the library's launch log on; return the names of the kernels it launched."""
    import ctypes
    from vae_amd import _lib as L
    lib = L.load()
    lib.vae_launch_log(1)
    try:
        fn()
    finally:
        lib.vae_launch_log(0)
    need = lib.vae_launch_log_names(None, 0)
    buf = ctypes.create_string_buffer(int(need))
    lib.vae_launch_log_names(buf, need)
    return buf.value.decode()
