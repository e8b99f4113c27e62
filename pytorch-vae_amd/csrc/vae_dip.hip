// DIP-VAE's covariance penalty on the batch's latent means, with its gradient (vaehip.h vae_dip_args;
// DIPVAE.loss_function, models/dip_vae.py:146-158, "DIP loss II").
//
//   c = mu - mean_d(mu) (per row), Cov = c^T c [D][D], s = mean_{i < min(B,D)} exp(2 lv[i][i]),
//   cov_z = Cov + s (every entry), dip = l_off sum_{j!=k} cov_z^2 + l_d sum_j (cov_z[j][j] - 1)^2,
//   G = d dip / d cov_z (symmetric), X = 2 c G, d dip / d mu = X - mean_d(X),
//   d dip / d lv[i][i] = (sum G) 2 exp(2 lv[i][i]) / min(B,D).
//
// Two launches.  dip_strip_kernel: a workgroup owns a strip of 16 columns of Cov, which is the same
// strip of G and of X.  It streams the centred rows through LDS twice: once with the batch as the k
// index (Cov strip = c^T c[:, strip], every wave a share of the 16-row tiles of the strip), then, G
// now in LDS, with the latent axis as the k index (X strip = 2 c G[:, strip], every wave a 16-row
// tile of the chunk; a batch that fits one chunk is not loaded again).  Both products run on
// v_mfma_f32_16x16x4_f32.  The strip's share of dip and of
// sum G leaves as doubles, X unreduced, and the strip's share of each row sum of X as a float.
// dip_finish_kernel: a workgroup per row adds the row-sum shares in strip order, subtracts the mean and
// writes / accumulates the gradient.  No atomics anywhere: two calls are bit-identical.
//
// LDS rows are D + 2 floats long.  For ds_read_b32 the bank is the dword address mod 32 within a
// 32-lane half: the batch-k product reads rows 8*(lane>>4) + step at column lane&15 (16*(lane>>4) +
// (lane&15) mod 32: distinct), the latent-k product row lane&15 at column lane>>4 (2*(lane&15) +
// (lane>>4) mod 32: distinct).
#include "vae_common.hpp"

namespace vae {
namespace {

constexpr int DIP_STRIP = 16;                      // columns of Cov / G / X per workgroup
constexpr int DIP_NT = 256;                        // threads of either kernel
constexpr int DIP_NW = DIP_NT / 64;
constexpr int DIP_CHUNK_FLOATS = 64 * (128 + 2);   // a chunk of rows: 64 x (D <= 128) or 32 x (D <= 256)
constexpr int DIP_DMAX = 256;

struct DipK {
  vae_dip_args a;
  double* partials;                                // [strips][2] = {dip share, sum-G share}
  float* rowsum;                                   // [strips][batch]: share of sum_d X[b][d]
};

__device__ __forceinline__ int dip_chunk_rows(int D) { return D <= 128 ? 64 : 32; }

// rows b0 .. b0+RB-1 of mu into `cs` [RB][D+2], centred over the latent axis; rows >= B are zero
__device__ __forceinline__ void dip_load_chunk(const vae_dip_args& a, float* cs, int b0, int RB) {
  const int B = a.batch, D = a.latent, LD = D + 2, tid = threadIdx.x;
  // (8 loads per thread in flight at once: the trip count depends on D, so the loop is unrolled by hand)
  const int total = RB * (D / 2);
  for (int v0 = tid; v0 < total; v0 += 8 * DIP_NT) {
    float2 m[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int v = v0 + u * DIP_NT;
      const int r = v / (D / 2), d2 = v - r * (D / 2);
      m[u] = float2{0.f, 0.f};
      if (v < total && b0 + r < B) m[u] = *reinterpret_cast<const float2*>(a.mulv + (long)(b0 + r) * 2 * D + 2 * d2);
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int v = v0 + u * DIP_NT;
      const int r = v / (D / 2), d2 = v - r * (D / 2);
      if (v < total) *reinterpret_cast<float2*>(cs + r * LD + 2 * d2) = m[u];
    }
  }
  __syncthreads();
  // row means: 4 threads per row, each a strided quarter of it, combined in a fixed order
  {
    const int r = tid >> 2, part = tid & 3;
    if (r < RB) {
      float s = 0.f;
      for (int d = part; d < D; d += 4) s += cs[r * LD + d];
      s += __shfl_xor(s, 1);
      s += __shfl_xor(s, 2);
      const float mean = s / (float)D;
      const bool live = b0 + r < B;
      for (int d = part; d < D; d += 4) cs[r * LD + d] = live ? cs[r * LD + d] - mean : 0.f;
    }
  }
  __syncthreads();
}

// s = mean_{i < n} exp(2 lv[i][i]), n = min(B, D) <= 256: one element per thread, waves in order
__device__ __forceinline__ float dip_diag_mean(const vae_dip_args& a, float* wsum) {
  const int B = a.batch, D = a.latent, n = B < D ? B : D, tid = threadIdx.x;
  float e = 0.f;
  if (tid < n) e = expf(2.f * a.mulv[(long)tid * 2 * D + D + tid]);
  for (int off = 32; off > 0; off >>= 1) e += __shfl_xor(e, off);
  if ((tid & 63) == 0) wsum[tid >> 6] = e;
  __syncthreads();
  const float s = (((wsum[0] + wsum[1]) + wsum[2]) + wsum[3]) / (float)n;
  __syncthreads();
  return s;
}

__global__ void __launch_bounds__(DIP_NT) dip_strip_kernel(DipK k) {
  const vae_dip_args& a = k.a;
  __shared__ __attribute__((aligned(16))) float cs[DIP_CHUNK_FLOATS];
  __shared__ float gs[DIP_DMAX * DIP_STRIP];       // G[j][strip column]
  __shared__ float wsum[DIP_NW];
  __shared__ double dsum[DIP_NW][2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int kg = lane >> 4, lc = lane & 15;
  const int B = a.batch, D = a.latent, LD = D + 2;
  const int RB = dip_chunk_rows(D);
  const int k0 = blockIdx.x * DIP_STRIP;           // first column of the strip
  constexpr int JT = DIP_DMAX / 16 / DIP_NW;       // 16-row tiles of the strip per wave, at most

  const float s = dip_diag_mean(a, wsum);

  // ---- Cov[16 jt + 4 kg + r][k0 + lc], jt = wave + NW i: k runs over the batch
  f32x4 cov[JT];
#pragma unroll
  for (int i = 0; i < JT; ++i) cov[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int b0 = 0; b0 < B; b0 += RB) {
    dip_load_chunk(a, cs, b0, RB);
    for (int bb = 0; bb < RB; bb += 32) {
#pragma unroll
      for (int st = 0; st < 8; ++st) {
        const float* row = cs + (bb + 8 * kg + st) * LD;
        const float bv = row[k0 + lc];
#pragma unroll
        for (int i = 0; i < JT; ++i) {
          const int jt = wave + DIP_NW * i;
          if (16 * jt < D) cov[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(row[16 * jt + lc], bv, cov[i], 0, 0, 0);
        }
      }
    }
    __syncthreads();                               // chunk consumed
  }

  // ---- G and the strip's share of dip and of sum G
  double dip = 0.0, gsum = 0.0;
#pragma unroll
  for (int i = 0; i < JT; ++i) {
    const int jt = wave + DIP_NW * i;
    if (16 * jt < D) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int j = 16 * jt + 4 * kg + r;
        const float cz = cov[i][r] + s;
        float g, t;
        if (j == k0 + lc) { t = cz - 1.f; g = 2.f * a.lambda_diag * t; t = a.lambda_diag * t * t; }
        else { g = 2.f * a.lambda_offdiag * cz; t = a.lambda_offdiag * cz * cz; }
        gs[j * DIP_STRIP + lc] = g;
        dip += (double)t;
        gsum += (double)g;
      }
    }
  }
  for (int off = 32; off > 0; off >>= 1) { dip += __shfl_xor(dip, off); gsum += __shfl_xor(gsum, off); }
  if (lane == 0) { dsum[wave][0] = dip; dsum[wave][1] = gsum; }
  __syncthreads();                                 // gs and dsum complete
  if (tid == 0) {
    double d = 0.0, g = 0.0;
    for (int w = 0; w < DIP_NW; ++w) { d += dsum[w][0]; g += dsum[w][1]; }
    k.partials[2 * blockIdx.x] = d;
    k.partials[2 * blockIdx.x + 1] = g;
  }

  // ---- X[b0 + 16 wave + 4 kg + r][k0 + lc] = 2 sum_j c[b][j] G[j][k0 + lc]: k runs over the latent axis
  for (int b0 = 0; b0 < B; b0 += RB) {
    if (B > RB) dip_load_chunk(a, cs, b0, RB);     // (a batch of one chunk is still in LDS, centred)
    if (16 * wave < RB) {
      f32x4 x = {0.f, 0.f, 0.f, 0.f};
      const float* row = cs + (16 * wave + lc) * LD + kg;
      const float* gcol = gs + kg * DIP_STRIP + lc;
      for (int j0 = 0; j0 < D; j0 += 4)
        x = __builtin_amdgcn_mfma_f32_16x16x4f32(row[j0], gcol[j0 * DIP_STRIP], x, 0, 0, 0);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int b = b0 + 16 * wave + 4 * kg + r;
        const float v = 2.f * x[r];
        float rs = v;                              // sum over the strip's 16 columns (lanes lc)
        rs += __shfl_xor(rs, 1); rs += __shfl_xor(rs, 2); rs += __shfl_xor(rs, 4); rs += __shfl_xor(rs, 8);
        if (b < B) {
          a.dmulv_dip[(long)b * 2 * D + k0 + lc] = v;
          if (lc == 0) k.rowsum[(long)blockIdx.x * B + b] = rs;
        }
      }
    }
    __syncthreads();                               // chunk consumed
  }
}

// row b: dmu = grad_scale (X - mean_d X), dlog_var = grad_scale (sum G) 2 exp(2 lv[b][b]) / n on the
// diagonal entry of rows b < n = min(B, D), zero elsewhere
__global__ void __launch_bounds__(DIP_NT) dip_finish_kernel(DipK k, int strips) {
  const vae_dip_args& a = k.a;
  const int B = a.batch, D = a.latent, n = B < D ? B : D;
  const int b = blockIdx.x, tid = threadIdx.x;
  float rs = 0.f;
  double gsum = 0.0;
  for (int t = 0; t < strips; ++t) { rs += k.rowsum[(long)t * B + b]; gsum += k.partials[2 * t + 1]; }
  const float mean = rs / (float)D;
  float* out = a.dmulv_dip + (long)b * 2 * D;
  float* acc = a.dmulv ? a.dmulv + (long)b * 2 * D : nullptr;
  for (int d = tid; d < 2 * D; d += DIP_NT) {
    float v;
    if (d < D) v = a.grad_scale * (out[d] - mean);
    else if (d - D == b && b < n) v = a.grad_scale * ((float)gsum * (2.f * expf(2.f * a.mulv[(long)b * 2 * D + d])) / (float)n);
    else v = 0.f;
    out[d] = v;
    if (acc) acc[d] += v;                          // one thread owns each element: a plain add
  }
}

int dip_check(const vae_dip_args* a, const char* what) {
  if (!a) return fail(VAE_E_BADARG, "%s: null args", what);
  if (a->batch < 1) return fail(VAE_E_BADSHAPE, "%s: batch %d is below 1", what, a->batch);
  if (a->batch > 1024) return fail(VAE_E_BADSHAPE, "%s: batch %d is above 1024", what, a->batch);
  if (a->latent <= 0 || a->latent % 32)
    return fail(VAE_E_BADSHAPE, "%s: latent %d is not a positive multiple of 32", what, a->latent);
  if (a->latent > DIP_DMAX) return fail(VAE_E_BADSHAPE, "%s: latent %d is above %d", what, a->latent, DIP_DMAX);
  return VAE_OK;
}

inline size_t dip_ws_bytes(const vae_dip_args* a) {
  const size_t strips = (size_t)a->latent / DIP_STRIP;
  return strips * 2 * sizeof(double) + strips * (size_t)a->batch * sizeof(float);
}

}  // namespace
}  // namespace vae

using namespace vae;

extern "C" int vae_dip_workspace_size(const vae_dip_args* a, size_t* bytes, int32_t* tiles) {
  if (!bytes) return fail(VAE_E_BADARG, "dip_workspace_size: null argument");
  if (int rc = dip_check(a, "dip_workspace_size")) return rc;
  *bytes = dip_ws_bytes(a);
  if (tiles) *tiles = a->latent / DIP_STRIP;
  return VAE_OK;
}

extern "C" int vae_dip_fwd(const vae_dip_args* a, void* stream) {
  if (int rc = dip_check(a, "dip_fwd")) return rc;
  if (!a->mulv || !a->dmulv_dip || !a->workspace) return fail(VAE_E_BADARG, "dip_fwd: mulv / dmulv_dip / workspace");
  if ((reinterpret_cast<uintptr_t>(a->mulv) & 7) || (reinterpret_cast<uintptr_t>(a->workspace) & 7))
    return fail(VAE_E_BADARG, "dip_fwd: mulv and the workspace must be 8-byte aligned");
  const long need = (long)dip_ws_bytes(a);
  if (a->workspace_bytes < need)
    return fail(VAE_E_BADARG, "dip_fwd: workspace of %ld bytes < %ld required (see vae_dip_workspace_size)",
                (long)a->workspace_bytes, need);
  const int strips = a->latent / DIP_STRIP;
  double* partials = static_cast<double*>(a->workspace);
  DipK k{*a, partials, reinterpret_cast<float*>(partials + 2 * strips)};
  hipStream_t st = (hipStream_t)stream;
  VAE_LAUNCH(dip_strip_kernel, dim3(strips), dim3(DIP_NT), 0, st, k);
  VAE_LAUNCH(dip_finish_kernel, dim3(a->batch), dim3(DIP_NT), 0, st, k, strips);
  return check_launch("dip_fwd");
}
