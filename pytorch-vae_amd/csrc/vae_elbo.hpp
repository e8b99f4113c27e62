// ELBO of the VAE family on one workgroup (vaehip.h vae_elbo_fwd; vanilla_vae.py:124-146,
// beta_vae.py:129-152, iwae.py:129-160, vq_vae.py:194-211, info_vae.py:128-148, dip_vae.py:125-164,
// miwae.py:132-164).
#pragma once
#include "vae_common.hpp"

namespace vae {

// One importance-weighted group of K rows (IWAE's S samples of an image, one of MIWAE's M estimates):
// Σ_k w lw with w = softmax_k(lw), lw_k = sse_k/img + kk (kk = M_N*kld_b), and the group's backward
// seeds g_k = w_k (1 + lw_k - Σ w lw) / groups into head_coef / kl_coef at row r0 + k.  REG: K <=
// ELBO_KREG, each sse read once and lw / exp kept in registers; else every pass recomputes them.
constexpr int ELBO_KREG = 8;

template <bool REG>
__device__ __forceinline__ float elbo_group(const vae_elbo_args& a, const float* sse, long r0, int K, float kk,
                                            float inv_img, float groups) {
  if constexpr (REG) {
    float lw[ELBO_KREG], e[ELBO_KREG];
    float mx = -INFINITY;
#pragma unroll
    for (int k = 0; k < ELBO_KREG; ++k)
      if (k < K) { lw[k] = sse[k] * inv_img + kk; mx = fmaxf(mx, lw[k]); }
    float den = 0.f;
#pragma unroll
    for (int k = 0; k < ELBO_KREG; ++k)
      if (k < K) { e[k] = expf(lw[k] - mx); den += e[k]; }
    float wl = 0.f;
#pragma unroll
    for (int k = 0; k < ELBO_KREG; ++k)
      if (k < K) wl += e[k] / den * lw[k];
#pragma unroll
    for (int k = 0; k < ELBO_KREG; ++k)
      if (k < K) {
        const float w = e[k] / den;
        const float g = w * (1.f + lw[k] - wl) / groups;        // dL/dlw
        a.head_coef[r0 + k] = g * 2.f * inv_img;
        a.kl_coef[r0 + k] = g * a.kld_weight;
      }
    return wl;
  } else {
    float mx = -INFINITY;
    for (int k = 0; k < K; ++k) mx = fmaxf(mx, sse[k] * inv_img + kk);
    float den = 0.f;
    for (int k = 0; k < K; ++k) den += expf(sse[k] * inv_img + kk - mx);
    float wl = 0.f;
    for (int k = 0; k < K; ++k) {
      const float lw = sse[k] * inv_img + kk;
      wl += expf(lw - mx) / den * lw;
    }
    for (int k = 0; k < K; ++k) {
      const float lw = sse[k] * inv_img + kk;
      const float w = expf(lw - mx) / den;
      const float g = w * (1.f + lw - wl) / groups;             // dL/dlw
      a.head_coef[r0 + k] = g * 2.f * inv_img;
      a.kl_coef[r0 + k] = g * a.kld_weight;
    }
    return wl;
  }
}

// kld_b = -0.5 Σ_d (1 + lv - mu^2 - exp(lv)) of row b = b0 + (threadIdx.x >> 2), one pass of a
// 256-thread workgroup over 64 rows of mulv [B][2*D]: 4 threads per row, each a quarter of the latent
// dims with all its loads in flight at once.  Every one of a row's 4 threads returns kld_b (0 past
// the batch).  The one home of this arithmetic: elbo_block below and vae_logcosh_loss call it.
__device__ __forceinline__ float kld_row_pass(const float* mulv, int B, int D, int b0) {
  const int part = threadIdx.x & 3, per = (D + 3) / 4;
  const int b = b0 + (threadIdx.x >> 2);
  float s = 0.f;
  if (b < B) {
    const float* mu = mulv + (long)b * 2 * D;
    const float* lv = mu + D;
    const int d0 = part * per, d1 = min(D, d0 + per);
#pragma unroll 32
    for (int d = d0; d < d1; ++d) s += 1.f + lv[d] - mu[d] * mu[d] - expf(lv[d]);
  }
  s += __shfl_xor(s, 1);
  s += __shfl_xor(s, 2);
  return -0.5f * s;
}

// The loss of vaehip.h vae_elbo_fwd by one 256-thread workgroup (kld_row: 1024 floats of LDS, red:
// 16) — run by elbo_kernel, and by the head backward's slab-reduction launch when the step fuses it
// (vae_head_args.elbo).
__device__ __forceinline__ void elbo_block(const vae_elbo_args& a, float* kld_row, float (*red)[4]) {
  const int B = a.batch, S = a.samples > 0 ? a.samples : 1, D = a.latent;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  // kld_b of every row (kld_row_pass: 64 rows per pass)
  if (a.kind != VAE_LOSS_VQ) {
    for (int b0 = 0; b0 < B; b0 += 64) {
      const int b = b0 + (threadIdx.x >> 2);
      const float k = kld_row_pass(a.mulv, B, D, b0);
      if ((threadIdx.x & 3) == 0 && b < B) kld_row[b] = k;
    }
  }
  __syncthreads();
  const float inv_img = 1.f / (float)a.img_elems;
  // totals: Σ sse, Σ kld_b
  float ts = 0.f, tk = 0.f;
  for (int i = threadIdx.x; i < B * S; i += 256) ts += a.sse[i];
  for (int b = threadIdx.x; b < B && a.kind != VAE_LOSS_VQ; b += 256) tk += kld_row[b];
  for (int off = 32; off > 0; off >>= 1) { ts += __shfl_xor(ts, off); tk += __shfl_xor(tk, off); }
  if (lane == 0) { red[0][wv] = ts; red[1][wv] = tk; }
  __syncthreads();
  const float sse_tot = red[0][0] + red[0][1] + red[0][2] + red[0][3];
  const float kld_mean = (red[1][0] + red[1][1] + red[1][2] + red[1][3]) / (float)B;
  for (int i = threadIdx.x; i < B * S; i += 256) a.per_img[i] = a.sse[i] * inv_img;

  if (a.kind == VAE_LOSS_VQ) {                  // vq_vae.py:203-211
    const float recon = sse_tot / ((float)B * (float)a.img_elems);
    const float vq = (1.f + a.vq_beta) * (*a.vq_sse) / a.vq_elems;
    if (threadIdx.x == 0) { a.out[0] = recon + vq; a.out[1] = recon; a.out[2] = vq; a.out[3] = 0.f; }
    return;
  }
  if (a.kind == VAE_LOSS_DIP) {
    // dip_vae.py:141-164: recon and kld are sums; the DIP term is the vae_dip partials (the first
    // double of each tile's pair) added in tile order by every thread
    double dip_d = 0.0;
    for (int t = 0; t < a.mmd_tiles; ++t) dip_d += a.mmd_partials[2 * t];
    const float dip = (float)dip_d;
    const float kld_sum = red[1][0] + red[1][1] + red[1][2] + red[1][3];
    for (int i = threadIdx.x; i < B; i += 256) { a.head_coef[i] = 2.f; a.kl_coef[i] = a.kld_weight; }
    if (threadIdx.x == 0) {
      a.out[0] = sse_tot + a.kld_weight * kld_sum + dip; a.out[1] = sse_tot; a.out[2] = -kld_sum; a.out[3] = kld_sum;
      a.mmd_out[0] = dip;
    }
    return;
  }
  if (a.kind != VAE_LOSS_IWAE && a.kind != VAE_LOSS_MIWAE) {
    const float recon = sse_tot / ((float)B * (float)a.img_elems);
    float loss, klc, kld_report;
    float rw = 1.f;                               // weight of the reconstruction term (and its seed)
    if (a.kind == VAE_LOSS_VANILLA) {
      loss = recon + a.kld_weight * kld_mean; klc = a.kld_weight; kld_report = -kld_mean;
    } else if (a.kind == VAE_LOSS_INFO) {
      // info_vae.py:141-148: the MMD term is the vae_mmd partials added in tile order (doubles, so
      // S_pp + S_zz - 2 S_pz keeps its digits through the cancellation); every thread adds them
      double pp = 0.0, zz = 0.0, pz = 0.0;
      for (int t = 0; t < a.mmd_tiles; ++t) {
        pp += a.mmd_partials[4 * t]; zz += a.mmd_partials[4 * t + 1]; pz += a.mmd_partials[4 * t + 2];
      }
      const float mmd = (float)(pp + zz - 2.0 * pz);
      rw = a.recon_weight;
      klc = a.kl_factor * a.kld_weight;
      loss = rw * recon + klc * kld_mean + a.mmd_coef * mmd;
      kld_report = -kld_mean;
      if (threadIdx.x == 0) a.mmd_out[0] = mmd;
    } else if (a.kind == VAE_LOSS_BETA_H) {
      loss = recon + a.beta * a.kld_weight * kld_mean; klc = a.beta * a.kld_weight; kld_report = kld_mean;
    } else {
      const float it = a.iter ? *a.iter : 1.f;
      const float C = fminf(fmaxf(a.c_max / a.c_stop_iter * it, 0.f), a.c_max);
      const float dlt = kld_mean - C;
      loss = recon + a.gamma * a.kld_weight * fabsf(dlt);
      klc = a.gamma * a.kld_weight * (dlt > 0.f ? 1.f : (dlt < 0.f ? -1.f : 0.f));
      kld_report = kld_mean;
    }
    const float hc = rw * 2.f / ((float)B * (float)a.img_elems);
    for (int i = threadIdx.x; i < B; i += 256) { a.head_coef[i] = hc; a.kl_coef[i] = klc / (float)B; }
    if (threadIdx.x == 0) { a.out[0] = loss; a.out[1] = recon; a.out[2] = kld_report; a.out[3] = kld_mean; }
    return;
  }
  // IWAE / MIWAE (iwae.py:129-160, miwae.py:148-164): the B*M groups of K rows, row b*M*K + m*K + k
  // (IWAE: M = 1, K = S); a thread owns a group.  lw = sse/img + M_N*kld_b ; w = softmax_k(lw) ;
  // loss = mean over the groups of Σ_k w lw
  const int M = a.kind == VAE_LOSS_MIWAE && a.mmd_tiles > 0 ? a.mmd_tiles : 1;
  const int K = S / M, G = B * M;
  float lsum = 0.f;
  for (int g = threadIdx.x; g < G; g += 256) {
    const int b = g / M;
    const float* sse = a.sse + (long)g * K;
    const float kk = a.kld_weight * kld_row[b];
    if (K <= ELBO_KREG) lsum += elbo_group<true>(a, sse, (long)g * K, K, kk, inv_img, (float)G);
    else lsum += elbo_group<false>(a, sse, (long)g * K, K, kk, inv_img, (float)G);
  }
  for (int off = 32; off > 0; off >>= 1) lsum += __shfl_xor(lsum, off);
  __syncthreads();
  if (lane == 0) red[2][wv] = lsum;
  __syncthreads();
  if (threadIdx.x == 0) {
    a.out[0] = (red[2][0] + red[2][1] + red[2][2] + red[2][3]) / (float)G;
    a.out[1] = sse_tot * inv_img / (float)(B * S);
    a.out[2] = -kld_mean;
    a.out[3] = kld_mean;
  }
}

}  // namespace vae
