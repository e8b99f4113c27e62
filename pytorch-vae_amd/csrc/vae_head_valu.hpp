// Decoder head on the VALU: the route of vae_head.hip's entry points for every call its MFMA
// kernels decline (fp32, images that are not 64 wide, widths other than 32 / 64 / 128, a data
// gradient without the BatchNorm epilogue).  Final Conv2d(C->3)+Tanh+SSE and its backward, one
// 256-pixel tile per workgroup with the input tile staged once in LDS.  Also the argument checks
// both routes share (head_setup) and the deterministic mode's slab (head_det).
#pragma once
#include "vae_common.hpp"

namespace vae {
namespace {

constexpr int HEAD_MAXC = 512;     // channels entering the head (the Autoencoder's widest final layer:
                                   // configs/patient_vvbig_ae.yaml, hidden_dims[0] = 512)
constexpr int HEAD_CW = 32;        // channels staged per pass when the input has more than 64
constexpr int HEAD_T = 256;        // threads = pixels per tile
constexpr int CO = 3;              // RGB
constexpr int HEAD_GS = 774;       // max (rows+2)*(w+2) with rows*w == 256

struct HeadP {
  int n, h, w, c, rows, samples, tiles;
  const void* x; vae_xform xf;
  const float* wt; const float* bias; const float* target;
  float* recon; float* sse; const float* coef;
  void* dx; vae_xform epi; float* dgamma; float* dbeta;
  int sum_reps, sum_rstride;
  float* dw; float* db;
  const float* grad_recon;
  float* det_slab;           // deterministic calls: per-workgroup partial rows (OrdSum)
};

__device__ __forceinline__ float act_of(const vae_xform& xf, const float* ta, const float* tb, float v, int ch) {
  if (xf.kind == VAE_X_BN_ACT) return lrelu(fmaf(v, ta[ch], tb[ch]), xf.slope);
  if (xf.kind == VAE_X_ACT) return lrelu(v, xf.slope);
  return v;
}

// BN forward coefficients of the head input (and x̂ = y*p + q for the backward epilogue);
// `update_running`: this block also applies the BatchNorm running-stat update (once per call)
__device__ void head_coefs(const vae_xform& xf, float* ta, float* tb, float* tp, float* tq,
                           bool update_running = false) {
  if (xf.kind != VAE_X_BN_ACT) return;
  if (xf.table) {
    const int C = xf.channels;
    for (int ch = threadIdx.x; ch < C; ch += blockDim.x) {
      ta[ch] = xf.table[ch]; tb[ch] = xf.table[C + ch];
      if (tp) { tp[ch] = xf.table[2 * C + ch]; tq[ch] = xf.table[3 * C + ch]; }
    }
    return;
  }
  for (int ch = threadIdx.x; ch < xf.channels; ch += blockDim.x) {
    BnMom mo;
    bn_moments(xf, ch, mo.mean, mo.invstd, mo.var);
    const BnFwd f = bn_fwd(mo, xf.gamma[ch]);
    ta[ch] = f.a;
    tb[ch] = f.b(xf.beta[ch]);
    if (tp) { tp[ch] = f.p; tq[ch] = f.q; }
    if (update_running && xf.running_mean) {
      const float unb = bn_unbiased(mo, xf);
      xf.running_mean[ch] = bn_momentum(xf, xf.running_mean[ch], mo.mean);
      xf.running_var[ch] = bn_momentum(xf, xf.running_var[ch], unb);
    }
  }
}

// Channels staged per pass: all of them up to 32 (one tile of (rows+2) x (w+2) x (c+4) floats),
// HEAD_CW at a time above (a 64-channel tile of a 64-wide image is already 105 KB)
__host__ __device__ inline int head_cw(int c) { return c > 32 ? HEAD_CW : c; }

// Stage act(x) rows [h0-1, h0+rows] x cols [-1, w], channels [c0, c0+cw) into LDS as
// [(rows+2)][(w+2)][cw+4] floats
template <class T>
__device__ void stage_input(const HeadP& p, int n, int h0, float* xs, const float* ta, const float* tb, int c0,
                            int cw) {
  const int CP = cw + 4, WP = p.w + 2;
  const int oct_per_pix = cw / 8;
  const int total = (p.rows + 2) * WP * oct_per_pix;
  const T* X = static_cast<const T*>(p.x);
  for (int e = threadIdx.x; e < total; e += blockDim.x) {
    const int o = e % oct_per_pix;
    const int pix = e / oct_per_pix;
    const int cc = pix % WP, rr = pix / WP;
    const int hi = h0 + rr - 1, wi = cc - 1;
    float v[8];
    if (hi >= 0 && hi < p.h && wi >= 0 && wi < p.w) {
      ld8(X + (((long)n * p.h + hi) * p.w + wi) * p.c + c0 + o * 8, v);
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = act_of(p.xf, ta, tb, v[j], c0 + o * 8 + j);
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = 0.f;
    }
    float* d = xs + (rr * WP + cc) * CP + o * 8;
    *reinterpret_cast<f32x4*>(d) = f32x4{v[0], v[1], v[2], v[3]};
    *reinterpret_cast<f32x4*>(d + 4) = f32x4{v[4], v[5], v[6], v[7]};
  }
}

// recon = tanh(conv3x3(act(x)) + b) -> NCHW; sse[n] += Σ (recon - target)^2
template <class T>
__global__ void __launch_bounds__(HEAD_T) head_fwd_kernel(HeadP p) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  __shared__ float ta[HEAD_MAXC], tb[HEAD_MAXC], ws[CO * 9 * 64], red[HEAD_T / 64];
  const int tiles_per_img = p.h / p.rows;
  const int n = blockIdx.x / tiles_per_img, h0 = (blockIdx.x % tiles_per_img) * p.rows;
  head_coefs(p.xf, ta, tb, nullptr, nullptr, blockIdx.x == 0);
  const int cw = head_cw(p.c);
  const int CP = cw + 4, WP = p.w + 2;
  const int tr = threadIdx.x / p.w, tc = threadIdx.x % p.w;
  float o[CO] = {p.bias[0], p.bias[1], p.bias[2]};
  for (int c0 = 0; c0 < p.c; c0 += cw) {
    __syncthreads();                                 // tables / the previous pass's reads
    for (int i = threadIdx.x; i < CO * 9 * cw; i += blockDim.x) {   // weights [co][tap][c0 .. c0+cw)
      const int ct = i / cw, c = i - ct * cw;
      ws[i] = p.wt[ct * p.c + c0 + c];
    }
    stage_input<T>(p, n, h0, smem, ta, tb, c0, cw);
    __syncthreads();
    for (int r = 0; r < 3; ++r)
      for (int s = 0; s < 3; ++s) {
        const float* xp = smem + ((tr + r) * WP + tc + s) * CP;
        const float* wp = ws + (r * 3 + s) * cw;
        for (int c = 0; c < cw; c += 4) {
          const f32x4 xv = *reinterpret_cast<const f32x4*>(xp + c);
#pragma unroll
          for (int co = 0; co < CO; ++co) {
            const float* wq = wp + co * 9 * cw + c;
            o[co] = fmaf(xv[0], wq[0], fmaf(xv[1], wq[1], fmaf(xv[2], wq[2], fmaf(xv[3], wq[3], o[co]))));
          }
        }
      }
  }
  const int hh = h0 + tr;
  const int img_t = n / p.samples;
  float sq = 0.f;
#pragma unroll
  for (int co = 0; co < CO; ++co) {
    const float y = tanhf(o[co]);
    const long oi = (((long)n * CO + co) * p.h + hh) * p.w + tc;
    p.recon[oi] = y;
    const float d = y - p.target[(((long)img_t * CO + co) * p.h + hh) * p.w + tc];
    sq = fmaf(d, d, sq);
  }
  for (int off = 32; off > 0; off >>= 1) sq += __shfl_xor(sq, off);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = sq;
  __syncthreads();
  if (threadIdx.x == 0) {
    float t = 0.f;
    for (int i = 0; i < HEAD_T / 64; ++i) t += red[i];
    if (p.det_slab) p.det_slab[blockIdx.x] = t;
    else atomicAdd(p.sse + n, t);
  }
}

// gseed = coef[img] * (recon - target) * (1 - recon^2)   (d loss / d pre-tanh)
__device__ __forceinline__ float gseed_at(const HeadP& p, int n, int co, int h, int w) {
  const long oi = (((long)n * CO + co) * p.h + h) * p.w + w;
  const float y = p.recon[oi];
  if (p.grad_recon) return p.grad_recon[oi] * (1.f - y * y);
  const float t = p.target[(((long)(n / p.samples) * CO + co) * p.h + h) * p.w + w];
  return p.coef[n] * (y - t) * (1.f - y * y);
}

// dx[h,w,c] = Σ_{r,s,co} gseed[h+1-r, w+1-s, co] · W[co][r][s][c], then the BN/LReLU backward
template <class T, int C>
__global__ void __launch_bounds__(HEAD_T) head_bwd_data_kernel(HeadP p) {
  __shared__ float ta[C], tb[C], tp[C], tq[C];
  __shared__ float ws[CO * 9 * C];
  __shared__ float gs[HEAD_GS * CO];                         // (rows+2) x (w+2) x 3
  __shared__ float r1[4][C], r2[4][C];
  const int tiles_per_img = p.h / p.rows;
  const int n = blockIdx.x / tiles_per_img, h0 = (blockIdx.x % tiles_per_img) * p.rows;
  head_coefs(p.epi, ta, tb, tp, tq);
  for (int i = threadIdx.x; i < CO * 9 * C; i += blockDim.x) ws[i] = p.wt[i];
  const int WP = p.w + 2;
  for (int e = threadIdx.x; e < (p.rows + 2) * WP; e += blockDim.x) {
    const int cc = e % WP, rr = e / WP;
    const int hi = h0 + rr - 1, wi = cc - 1;
    const bool in = hi >= 0 && hi < p.h && wi >= 0 && wi < p.w;
#pragma unroll
    for (int co = 0; co < CO; ++co) gs[e * CO + co] = in ? gseed_at(p, n, co, hi, wi) : 0.f;
  }
  __syncthreads();
  const int tr = threadIdx.x / p.w, tc = threadIdx.x % p.w;
  float da[C];
#pragma unroll
  for (int c = 0; c < C; ++c) da[c] = 0.f;
#pragma unroll 1
  for (int r = 0; r < 3; ++r)
#pragma unroll 1
    for (int s = 0; s < 3; ++s) {
      const float* g = gs + ((tr + 2 - r) * WP + (tc + 2 - s)) * CO;
#pragma unroll
      for (int co = 0; co < CO; ++co) {
        const float gv = g[co];
        const float* wq = ws + co * 9 * C + (r * 3 + s) * C;
#pragma unroll
        for (int c = 0; c < C; ++c) da[c] = fmaf(gv, wq[c], da[c]);
      }
    }
  // BN + LeakyReLU backward of the head input
  const long base = (((long)n * p.h + h0 + tr) * p.w + tc) * C;
  const T* Y = static_cast<const T*>(p.epi.aux);
  T* DX = static_cast<T*>(p.dx);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int c0 = 0; c0 < C; c0 += 8) {
    float y[8];
    if (p.epi.kind != VAE_X_NONE) ld8(Y + base + c0, y);
    else {
#pragma unroll
      for (int j = 0; j < 8; ++j) y[j] = 0.f;
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int c = c0 + j;
      float gv = da[c], s1 = 0.f, s2 = 0.f;
      if (p.epi.kind == VAE_X_BN_ACT) {
        const float z = fmaf(y[j], ta[c], tb[c]);
        gv = z > 0.f ? gv : gv * p.epi.slope;
        s1 = gv;
        s2 = gv * fmaf(y[j], tp[c], tq[c]);
      } else if (p.epi.kind == VAE_X_ACT) {
        gv = y[j] > 0.f ? gv : gv * p.epi.slope;
      }
      DX[base + c] = cvt<T>(gv);
      if (p.epi.kind == VAE_X_BN_ACT) {
        for (int off = 32; off > 0; off >>= 1) { s1 += __shfl_xor(s1, off); s2 += __shfl_xor(s2, off); }
        if (lane == 0) { r1[wv][c] = s1; r2[wv][c] = s2; }
      }
    }
  }
  if (p.epi.kind == VAE_X_BN_ACT) {
    __syncthreads();
    const long roff = p.sum_reps > 1 ? (long)(blockIdx.x % p.sum_reps) * p.sum_rstride : 0;
    for (int c = threadIdx.x; c < C; c += blockDim.x) {
      const float b = r1[0][c] + r1[1][c] + r1[2][c] + r1[3][c], g = r2[0][c] + r2[1][c] + r2[2][c] + r2[3][c];
      if (p.det_slab) {
        p.det_slab[(long)blockIdx.x * 2 * C + c] = b;
        p.det_slab[(long)blockIdx.x * 2 * C + C + c] = g;
      } else {
        atomicAdd(p.dbeta + roff + c, b);
        atomicAdd(p.dgamma + roff + c, g);
      }
    }
  }
}

// head_bwd_data_kernel for inputs wider than 64 channels (the Autoencoder's 128-512-channel final
// layers): the same sums, HEAD_CW channels at a time (a register accumulator per channel of the
// pass, the pass's weights in LDS)
template <class T>
__global__ void __launch_bounds__(HEAD_T) head_bwd_data_wide_kernel(HeadP p) {
  constexpr int CW = HEAD_CW;
  __shared__ float ta[HEAD_MAXC], tb[HEAD_MAXC], tp[HEAD_MAXC], tq[HEAD_MAXC];
  __shared__ float ws[CO * 9 * CW];
  __shared__ float gs[HEAD_GS * CO];
  __shared__ float r1[4][CW], r2[4][CW];
  const int C = p.c;
  const int tiles_per_img = p.h / p.rows;
  const int n = blockIdx.x / tiles_per_img, h0 = (blockIdx.x % tiles_per_img) * p.rows;
  head_coefs(p.epi, ta, tb, tp, tq);
  const int WP = p.w + 2;
  for (int e = threadIdx.x; e < (p.rows + 2) * WP; e += blockDim.x) {
    const int cc = e % WP, rr = e / WP;
    const int hi = h0 + rr - 1, wi = cc - 1;
    const bool in = hi >= 0 && hi < p.h && wi >= 0 && wi < p.w;
#pragma unroll
    for (int co = 0; co < CO; ++co) gs[e * CO + co] = in ? gseed_at(p, n, co, hi, wi) : 0.f;
  }
  const int tr = threadIdx.x / p.w, tc = threadIdx.x % p.w;
  const long base = (((long)n * p.h + h0 + tr) * p.w + tc) * C;
  const T* Y = static_cast<const T*>(p.epi.aux);
  T* DX = static_cast<T*>(p.dx);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const long roff = p.sum_reps > 1 ? (long)(blockIdx.x % p.sum_reps) * p.sum_rstride : 0;
  for (int c0 = 0; c0 < C; c0 += CW) {
    __syncthreads();                                 // gs / tables, and the previous pass's ws, r1, r2
    for (int i = threadIdx.x; i < CO * 9 * CW; i += blockDim.x) {
      const int ct = i / CW, c = i - ct * CW;
      ws[i] = p.wt[ct * C + c0 + c];
    }
    __syncthreads();
    float da[CW];
#pragma unroll
    for (int c = 0; c < CW; ++c) da[c] = 0.f;
#pragma unroll 1
    for (int r = 0; r < 3; ++r)
#pragma unroll 1
      for (int s = 0; s < 3; ++s) {
        const float* g = gs + ((tr + 2 - r) * WP + (tc + 2 - s)) * CO;
#pragma unroll
        for (int co = 0; co < CO; ++co) {
          const float gv = g[co];
          const float* wq = ws + co * 9 * CW + (r * 3 + s) * CW;
#pragma unroll
          for (int c = 0; c < CW; ++c) da[c] = fmaf(gv, wq[c], da[c]);
        }
      }
#pragma unroll
    for (int k0 = 0; k0 < CW; k0 += 8) {
      float y[8];
      if (p.epi.kind != VAE_X_NONE) ld8(Y + base + c0 + k0, y);
      else {
#pragma unroll
        for (int j = 0; j < 8; ++j) y[j] = 0.f;
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int c = c0 + k0 + j;
        float gv = da[k0 + j], s1 = 0.f, s2 = 0.f;
        if (p.epi.kind == VAE_X_BN_ACT) {
          const float z = fmaf(y[j], ta[c], tb[c]);
          gv = z > 0.f ? gv : gv * p.epi.slope;
          s1 = gv;
          s2 = gv * fmaf(y[j], tp[c], tq[c]);
        } else if (p.epi.kind == VAE_X_ACT) {
          gv = y[j] > 0.f ? gv : gv * p.epi.slope;
        }
        DX[base + c] = cvt<T>(gv);
        if (p.epi.kind == VAE_X_BN_ACT) {
          for (int off = 32; off > 0; off >>= 1) { s1 += __shfl_xor(s1, off); s2 += __shfl_xor(s2, off); }
          if (lane == 0) { r1[wv][k0 + j] = s1; r2[wv][k0 + j] = s2; }
        }
      }
    }
    if (p.epi.kind == VAE_X_BN_ACT) {
      __syncthreads();
      if (threadIdx.x < CW) {
        const int c = threadIdx.x;
        const float b = r1[0][c] + r1[1][c] + r1[2][c] + r1[3][c], g = r2[0][c] + r2[1][c] + r2[2][c] + r2[3][c];
        if (p.det_slab) {
          p.det_slab[(long)blockIdx.x * 2 * C + c0 + c] = b;
          p.det_slab[(long)blockIdx.x * 2 * C + C + c0 + c] = g;
        } else {
          atomicAdd(p.dbeta + roff + c0 + c, b);
          atomicAdd(p.dgamma + roff + c0 + c, g);
        }
      }
    }
  }
}

// dW[co][r][s][c] += Σ_pix gseed[pix][co] · act(x)[pix + (r-1, s-1)][c];  db[co] += Σ gseed
template <class T>
__global__ void __launch_bounds__(HEAD_T) head_bwd_filter_kernel(HeadP p) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  __shared__ float ta[HEAD_MAXC], tb[HEAD_MAXC], gs[HEAD_T * CO], red[CO][HEAD_T / 64];
  constexpr int NI = (9 * HEAD_MAXC + HEAD_T - 1) / HEAD_T;    // dW elements per thread
  const int nidx = 9 * p.c;
  const int cw = head_cw(p.c);
  float acc[NI][CO];
  float dbacc[CO] = {0.f, 0.f, 0.f};
#pragma unroll
  for (int i = 0; i < NI; ++i)
#pragma unroll
    for (int co = 0; co < CO; ++co) acc[i][co] = 0.f;
  head_coefs(p.xf, ta, tb, nullptr, nullptr);
  const int tiles_per_img = p.h / p.rows;
  const int CP = cw + 4, WP = p.w + 2;
  for (int tile = blockIdx.x; tile < p.tiles; tile += gridDim.x) {
    const int n = tile / tiles_per_img, h0 = (tile % tiles_per_img) * p.rows;
    __syncthreads();
    {
      const int tr = threadIdx.x / p.w, tc = threadIdx.x % p.w;
#pragma unroll
      for (int co = 0; co < CO; ++co) {
        const float g = gseed_at(p, n, co, h0 + tr, tc);
        gs[threadIdx.x * CO + co] = g;
        dbacc[co] += g;
      }
    }
    for (int c0 = 0; c0 < p.c; c0 += cw) {
      if (c0) __syncthreads();                       // the previous pass's reads of the tile
      stage_input<T>(p, n, h0, smem, ta, tb, c0, cw);
      __syncthreads();
#pragma unroll
      for (int i = 0; i < NI; ++i) {
        const int idx = threadIdx.x + i * HEAD_T;
        if (idx >= nidx) break;
        const int tap = idx / p.c, c = idx - tap * p.c;
        if (c < c0 || c >= c0 + cw) continue;        // (this pass stages channels [c0, c0+cw))
        const int r = tap / 3, s = tap - r * 3;
        for (int pix = 0; pix < HEAD_T; ++pix) {
          const int tr = pix / p.w, tc = pix - tr * p.w;
          const float xv = smem[((tr + r) * WP + tc + s) * CP + c - c0];
#pragma unroll
          for (int co = 0; co < CO; ++co) acc[i][co] = fmaf(gs[pix * CO + co], xv, acc[i][co]);
        }
      }
    }
  }
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    const int idx = threadIdx.x + i * HEAD_T;
    if (idx >= nidx) break;
#pragma unroll
    for (int co = 0; co < CO; ++co) {
      if (p.det_slab) p.det_slab[(long)blockIdx.x * (CO * nidx + CO) + co * nidx + idx] = acc[i][co];
      else atomicAdd(p.dw + co * nidx + idx, acc[i][co]);
    }
  }
  if (p.db) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int co = 0; co < CO; ++co) {
      float s = dbacc[co];
      for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
      if (lane == 0) red[co][wv] = s;
    }
    __syncthreads();
    if (threadIdx.x < CO) {
      float t = 0.f;
      for (int i = 0; i < HEAD_T / 64; ++i) t += red[threadIdx.x][i];
      if (p.det_slab) p.det_slab[(long)blockIdx.x * (CO * nidx + CO) + CO * nidx + threadIdx.x] = t;
      else atomicAdd(p.db + threadIdx.x, t);
    }
  }
}

int head_setup(const vae_head_args* a, HeadP& p, const char* what) {
  if (!a || !a->x || !a->wt || !a->bias || !a->target || !a->recon) return fail(VAE_E_BADARG, "%s: null tensor", what);
  if (a->c % 8 || a->c > HEAD_MAXC || a->c <= 0 || (a->c > 32 && a->c % HEAD_CW))
    return fail(VAE_E_UNSUPPORTED, "%s: channels %d", what, a->c);
  if (a->w <= 0 || a->w > 256 || HEAD_T % a->w || a->h % (HEAD_T / a->w))
    return fail(VAE_E_UNSUPPORTED, "%s: spatial %dx%d (need w | 256 and (256/w) | h)", what, a->h, a->w);
  if (a->dtype != VAE_F32 && a->dtype != VAE_BF16) return fail(VAE_E_BADDTYPE, "%s: dtype", what);
  if (a->deterministic && a->dtype != VAE_F32)
    return fail(VAE_E_UNSUPPORTED, "%s: deterministic reductions need dtype VAE_F32", what);
  memset(&p, 0, sizeof(p));
  p.n = a->n; p.h = a->h; p.w = a->w; p.c = a->c; p.rows = HEAD_T / a->w;
  p.samples = a->samples > 0 ? a->samples : 1;
  p.tiles = a->n * (a->h / p.rows);
  p.x = a->x; p.xf = a->x_xf; p.wt = a->wt; p.bias = a->bias; p.target = a->target;
  p.recon = a->recon; p.sse = a->sse; p.coef = a->coef;
  p.dx = a->dx; p.epi = a->dx_epi; p.dgamma = a->dx_dgamma; p.dbeta = a->dx_dbeta;
  p.sum_reps = a->sum_reps; p.sum_rstride = a->sum_rstride;
  p.dw = a->dw; p.db = a->db; p.grad_recon = a->grad_recon;
  if (p.xf.channels <= 0) p.xf.channels = a->c;
  if (p.epi.channels <= 0) p.epi.channels = a->c;
  return VAE_OK;
}

// A deterministic head call keeps its per-workgroup partials (`floats` of them) at the start of
// the workspace; the launcher adds them with ordered_sum_launch after its kernel.
int head_det(const vae_head_args* a, HeadP& p, long floats, const char* what) {
  if (!a->deterministic || floats <= 0) return VAE_OK;
  if (!a->workspace && !querying()) return fail(VAE_E_BADARG, "%s: a deterministic call needs a workspace", what);
  if (!ws_fits(floats * 4, a->workspace_bytes, what)) return VAE_E_BADARG;
  p.det_slab = static_cast<float*>(a->workspace);
  return VAE_OK;
}

// ---------------------------------------------------------------- the VALU route of each entry point
int head_fwd_valu(const vae_head_args* a, HeadP& p, hipStream_t st) {
  int rc;
  const size_t lds = (size_t)(p.rows + 2) * (p.w + 2) * (head_cw(p.c) + 4) * sizeof(float);
  if (lds > 64 * 1024) return fail(VAE_E_UNSUPPORTED, "head_fwd: tile too large");
  if ((rc = head_det(a, p, p.tiles, "head_fwd"))) return rc;
  if (a->dtype == VAE_F32) VAE_LAUNCH(head_fwd_kernel<float>, dim3(p.tiles), dim3(HEAD_T), lds, st, p);
  else VAE_LAUNCH(head_fwd_kernel<__bf16>, dim3(p.tiles), dim3(HEAD_T), lds, st, p);
  if ((rc = check_launch("head_fwd")) || !p.det_slab) return rc;
  OrdSum o;                                          // sse[n] += the image's tiles, in tile order
  memset(&o, 0, sizeof(o));
  o.slab = p.det_slab; o.rstride = 1; o.groups = p.n; o.rpg = p.h / p.rows; o.cols = 1; o.cw = 1; o.folds = 1;
  o.dst[0] = p.sse; o.gstride = 1;
  return ordered_sum_launch(o, st);
}

int head_bwd_data_valu(const vae_head_args* a, HeadP& p, hipStream_t st) {
  int rc;
  const bool f = a->dtype == VAE_F32;
  const bool sums = p.epi.kind == VAE_X_BN_ACT;
  if (sums && (rc = head_det(a, p, (long)p.tiles * 2 * p.c, "head_bwd_data"))) return rc;
  switch (a->c) {
    case 32:
      if (f) VAE_LAUNCH((head_bwd_data_kernel<float, 32>), dim3(p.tiles), dim3(HEAD_T), 0, st, p);
      else VAE_LAUNCH((head_bwd_data_kernel<__bf16, 32>), dim3(p.tiles), dim3(HEAD_T), 0, st, p);
      break;
    case 64:
      if (f) VAE_LAUNCH((head_bwd_data_kernel<float, 64>), dim3(p.tiles), dim3(HEAD_T), 0, st, p);
      else VAE_LAUNCH((head_bwd_data_kernel<__bf16, 64>), dim3(p.tiles), dim3(HEAD_T), 0, st, p);
      break;
    default:      // (head_setup: 64 < c <= HEAD_MAXC, c % HEAD_CW == 0)
      if (a->c <= 64) return fail(VAE_E_UNSUPPORTED, "head_bwd_data: channels %d (32, 64 or a multiple of %d)", a->c, HEAD_CW);
      if (f) VAE_LAUNCH((head_bwd_data_wide_kernel<float>), dim3(p.tiles), dim3(HEAD_T), 0, st, p);
      else VAE_LAUNCH((head_bwd_data_wide_kernel<__bf16>), dim3(p.tiles), dim3(HEAD_T), 0, st, p);
      break;
  }
  if ((rc = check_launch("head_bwd_data")) || !p.det_slab) return rc;
  OrdSum o;                                          // Σg, Σg·x̂ over the tiles, in tile order
  memset(&o, 0, sizeof(o));
  o.slab = p.det_slab; o.rstride = 2L * p.c; o.groups = 1; o.rpg = p.tiles; o.cols = 2 * p.c; o.cw = p.c;
  o.hstride = p.c; o.folds = 1; o.dst[0] = p.dbeta; o.dst[1] = p.dgamma;
  return ordered_sum_launch(o, st);
}

int head_bwd_filter_valu(const vae_head_args* a, HeadP& p, hipStream_t st) {
  int rc;
  const size_t lds = (size_t)(p.rows + 2) * (p.w + 2) * (head_cw(p.c) + 4) * sizeof(float);
  const int grid = p.tiles < 256 ? p.tiles : 256;
  const int nw = CO * 9 * p.c;                       // dW elements; db follows in a partial row
  if ((rc = head_det(a, p, (long)grid * (nw + CO), "head_bwd_filter"))) return rc;
  if (a->dtype == VAE_F32) VAE_LAUNCH(head_bwd_filter_kernel<float>, dim3(grid), dim3(HEAD_T), lds, st, p);
  else VAE_LAUNCH(head_bwd_filter_kernel<__bf16>, dim3(grid), dim3(HEAD_T), lds, st, p);
  if ((rc = check_launch("head_bwd_filter")) || !p.det_slab) return rc;
  OrdSum o;                                          // dW, db over the workgroups, in order
  memset(&o, 0, sizeof(o));
  o.slab = p.det_slab; o.rstride = nw + CO; o.groups = 1; o.rpg = grid; o.cols = p.db ? nw + CO : nw; o.cw = nw;
  o.hstride = nw; o.folds = 1; o.dst[0] = p.dw; o.dst[1] = p.db;
  return ordered_sum_launch(o, st);
}

}  // namespace
}  // namespace vae
