// The implicit-GEMM description (GemmParams) of each Conv2d / ConvTranspose2d problem, built from
// the C-ABI arguments in one place.  A Conv2d and a ConvTranspose2d are each other's data
// gradient, so there are two gathers, each told which tensor it reads and which it writes:
//   strided gather (A_CONV / B_GATHER): Conv2d forward, ConvTranspose2d data gradient, both
//                                       weight gradients, the stride-1 flipped Conv2d data gradient
//   phase gather (A_CONVT):             ConvTranspose2d forward, Conv2d data gradient
// and two epilogues (forward, backward).  Plain functions only: including this header adds no
// kernel to a translation unit.
#pragma once
#include "vae_igemm.hpp"

namespace vae {
namespace {

inline vae_xform sanitize(vae_xform x) {
  if (x.channels <= 0) x.channels = 1;
  return x;
}

inline GemmParams base_params() {
  GemmParams p;
  memset(&p, 0, sizeof(p));
  p.ksplit = 1; p.nphase = 1; p.ones_col = -1; p.gs = 1; p.samples = 1; p.gr = 1;
  p.a_xf.channels = 1; p.b_xf.channels = 1; p.epi_xf.channels = 1; p.res_xf.channels = 1;
  p.ntap_h[0] = p.ntap_h[1] = p.ntap_w[0] = p.ntap_w[1] = 1;
  return p;
}

// VAE_OK, or the code of the failure it has recorded (an entry returns it as it is).
inline int check_geom(const vae_conv_args* a, const char* what) {
  if (!a) return fail(VAE_E_BADARG, "%s: null args", what);
  if (a->n <= 0 || a->h <= 0 || a->w <= 0 || a->c <= 0 || a->k <= 0 || a->p <= 0 || a->q <= 0 || a->r <= 0 ||
      a->stride <= 0 || a->pad < 0)
    return fail(VAE_E_BADSHAPE, "%s: bad geometry", what);
  if (a->deterministic && a->dtype != VAE_F32)
    return fail(VAE_E_UNSUPPORTED, "%s: deterministic reductions need dtype VAE_F32", what);
  return VAE_OK;
}

// 1x1, stride 1, no padding: every output pixel reads its own input pixel
inline bool pointwise(const vae_conv_args* a) {
  return a->r == 1 && a->stride == 1 && a->pad == 0 && a->h == a->p && a->w == a->q;
}

// Phase tap tables of a transposed conv (or conv dgrad) with stride S, kernel R, padding P:
// output coordinate o of phase ph = o % S receives taps r with (ph + P - r) % S == 0.
inline bool make_taps(GemmParams& p, int S, int R, int P) {
  if (S < 1 || S > 2) return false;
  for (int ph = 0; ph < S; ++ph) {
    const int first = ((ph + P) % S + S) % S;       // smallest r with (ph + P - r) % S == 0
    const int n = first < R ? (R - 1 - first) / S + 1 : 0;
    if (n < 1 || n > 4) return false;
    p.tap0[ph] = first;
    p.ntap_h[ph] = n; p.ntap_w[ph] = n;
    p.tap_d[ph] = (ph + P - first) / S;
  }
  return true;
}

// Geometry of a strided-conv gather with kernel r, stride, padding `pad`.  of_dy = false: the
// layer input x [n][h][w][c] is read on the output grid p x q (Conv2d forward and weight
// gradient); of_dy = true: dy [n][p][q][k] is read on the input grid h x w (ConvTranspose2d data
// and weight gradient, and the stride-1 flipped Conv2d data gradient with pad = r-1-pad).  The
// phase gather starts from the same fields.
inline void strided_gather(GemmParams& p, const vae_conv_args* a, bool of_dy, int pad) {
  p.gn = a->n; p.gr = a->r; p.gs = a->stride; p.gpad = pad;
  if (!of_dy) { p.gh = a->h; p.gw = a->w; p.gc = a->c; p.gp = a->p; p.gq = a->q; }
  else { p.gh = a->p; p.gw = a->q; p.gc = a->k; p.gp = a->h; p.gq = a->w; }
}

// out[pixel][N] = Σ_{r,s,gc} gathered · weights[N][r][s][gc] (k-contiguous weight rows):
//   of_dy = false: y = conv(xf(x), W)      (vae_conv2d_fwd)
//   of_dy = true:  dx = conv(dy', weights) (vae_convT2d_bwd_data; the stride-1 flipped
//                  vae_conv2d_bwd_data with the flipped copy of W and pad = r-1-pad)
inline GemmParams strided_conv_params(const vae_conv_args* a, bool of_dy, const void* weights, int pad) {
  GemmParams p = base_params();
  p.det = a->deterministic;
  strided_gather(p, a, of_dy, pad);
  p.M = p.gn * p.gp * p.gq; p.N = of_dy ? a->c : a->k; p.K = p.gr * p.gr * p.gc;
  p.a_ptr = of_dy ? a->dy : a->x; p.a_xf = sanitize(of_dy ? a->dy_xf : a->x_xf);
  p.g_nchw = of_dy ? 0 : a->x_nchw_f32;
  p.b_ptr = weights; p.b_ld = p.K;
  p.out = of_dy ? a->dx : a->y; p.out_ld = p.N;
  return p;
}

// out[phase pixel][N] = Σ_{taps of the phase, gc} gathered · W: one GEMM per output phase
// (stride^2 of them) over the taps that reach it.
//   of_dy = false: y = convT(xf(x), W[c][r][s][k])  (vae_convT2d_fwd)
//   of_dy = true:  dx = convT(dy', W[k][r][s][c])   (vae_conv2d_bwd_data)
// B is the layer's own weights, read through the tap tables (rows of N); swapped_weights points
// it at the copy with the outer axes swapped instead.  False: stride / kernel without tap tables.
inline bool phase_gather_params(GemmParams& p, const vae_conv_args* a, bool of_dy) {
  const int S = a->stride;
  p = base_params();
  p.det = a->deterministic;
  if (!make_taps(p, S, a->r, a->pad)) return false;
  p.nphase = S * S;
  strided_gather(p, a, of_dy, a->pad);               // the same tensors; the grid written is cut
  p.gho = p.gp; p.gwo = p.gq;                         // into its phases
  p.gp = p.gho / S; p.gq = p.gwo / S;
  p.M = p.gn * p.gp * p.gq; p.N = of_dy ? a->c : a->k; p.K = 0;
  p.a_ptr = of_dy ? a->dy : a->x; p.a_xf = sanitize(of_dy ? a->dy_xf : a->x_xf);
  p.b_ptr = a->wt; p.b_ld = p.N; p.b_taps = 1;
  p.out = of_dy ? a->dx : a->y; p.out_ld = p.N; p.out_phase = 1;
  return true;
}

// ... against the swapped-axes copy WT[N][r][s][gc] (k-contiguous rows, as the conv-GEMM reads)
inline void swapped_weights(GemmParams& p, const void* wt_t) {
  p.b_ptr = wt_t; p.b_ld = p.gr * p.gr * p.gc; p.b_taps = 0;
}

// Forward epilogue: + bias, + xf(residual), per-channel Σ / Σ² for the next BatchNorm
inline void fwd_epilogue(GemmParams& p, const vae_conv_args* a) {
  p.bias = a->bias; p.sum = a->y_sum; p.sumsq = a->y_sumsq;
  p.sum_reps = a->sum_reps; p.sum_rstride = a->sum_rstride;
  p.residual = a->residual; p.res_xf = sanitize(a->residual_xf);
}

// Backward epilogue: [+ residual: the gradient through a skip connection], g = dx·act'(z) of the
// producing layer's BatchNorm / LeakyReLU (epi), Σg -> dβ, Σg·x̂ -> dγ
inline int bwd_epilogue(GemmParams& p, const vae_xform& epi, float* dgamma, float* dbeta, int sum_reps, int sum_rstride,
                        const void* residual, const char* what) {
  p.epi_xf = sanitize(epi); p.dgamma = dgamma; p.dbeta = dbeta;
  p.sum_reps = sum_reps; p.sum_rstride = sum_rstride;
  p.residual = residual;
  if (p.epi_xf.kind == VAE_X_BN_ACT && (!dgamma || !dbeta)) return fail(VAE_E_BADARG, "%s: dgamma/dbeta", what);
  return VAE_OK;
}

}  // namespace
}  // namespace vae
