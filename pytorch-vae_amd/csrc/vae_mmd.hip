// Maximum mean discrepancy of the latent batch against a prior sample, with its gradient
// (vaehip.h vae_mmd_args; InfoVAE.compute_mmd / compute_kernel, models/info_vae.py:150-229).
//
// The computation is attention-shaped over U = [z; prior] (2B rows of D floats): pairwise dot
// products U U^T, an elementwise kernel function, then weights x U for the gradient
//   dmmd/dz_a = sum_c coef[a][c] (U_c - z_a),  coef = +4w on latent columns, -4w on prior columns,
//   imq: w = k^2 / C;  rbf: w = k / (D sigma B^2).
// A workgroup owns 16 latent rows and the 16 prior rows of the same indices, whose fragments stay in
// registers for the whole kernel; the columns (every row of U) stream through LDS in tiles of 16 per
// wave.  Both products run on v_mfma_f32_16x16x4_f32.  The first one is taken TRANSPOSED —
// T[col][row], columns as the M operand — so that its output registers (lane l, register r: column
// 4*(l>>4)+r, row l&15) already are the A operand of the second product G[row][:] += coef^T U_cols
// with the k index permuted the same way on both operands; no transpose through LDS.
// d^2 = |a|^2 + |b|^2 - 2 a.b, clamped at 0; the same-set diagonal is recognised by index.
// The three sums are kept in double (they cancel in S_pp + S_zz - 2 S_pz) and leave the workgroup as
// one row of partials; the waves' gradient tiles meet in LDS and are added in wave order: no atomics.
#include "vae_common.hpp"
#include "vae_philox.hpp"

namespace vae {
namespace {

constexpr int MMD_ROWS = 16;                       // latent rows (and prior rows) per workgroup
constexpr float MMD_IMQ_EPS = 1e-7f;               // info_vae.py:198

struct MmdK {
  vae_mmd_args a;
  double* partials;
};

// z or prior elements [row][4*v4 .. +3] of U, by set
__device__ __forceinline__ f32x4 z_vec(const vae_mmd_args& a, int row, int v4) {
  const int D = a.latent;
  const f32x4 mu = *reinterpret_cast<const f32x4*>(a.mulv + (long)row * 2 * D + 4 * v4);
  const f32x4 lv = *reinterpret_cast<const f32x4*>(a.mulv + (long)row * 2 * D + D + 4 * v4);
  const f32x4 e = *reinterpret_cast<const f32x4*>(a.eps + (long)row * D + 4 * v4);
  f32x4 z;
#pragma unroll
  for (int i = 0; i < 4; ++i) z[i] = fmaf(e[i], expf(0.5f * lv[i]), mu[i]);      // as vae_reparam_fwd
  return z;
}
__device__ __forceinline__ f32x4 prior_vec(const vae_mmd_args& a, int row, int v4, uint32_t step) {
  if (a.prior_gen) return normal4_stream((uint32_t)(row * (a.latent / 4) + v4), step, kStreamPrior, a.prior_seed);
  return *reinterpret_cast<const f32x4*>(a.prior + (long)row * a.latent + 4 * v4);
}

// DMAX: largest latent size of the instantiation (register fragments of DMAX/4 floats per row set);
// NW waves, each scoring 16 of the NW*16 columns of a tile.
template <int DMAX, int NW>
__global__ void __launch_bounds__(64 * NW) mmd_kernel(MmdK k) {
  const vae_mmd_args& a = k.a;
  constexpr int SMAX = DMAX / 4;                   // k-steps: lane l supplies dims (l>>4)*S + s
  constexpr int CT = 16 * NW;                      // columns per tile
  constexpr int LDM = DMAX + 4;                    // padded LDS row: conflict-free fragment reads
  constexpr int NT = 64 * NW;
  __shared__ __attribute__((aligned(16))) float cols[CT * LDM];     // column tile; later the waves' G
  __shared__ float cn[CT];
  __shared__ float rs[NW][16];
  __shared__ double sums[NW][3];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int kg = lane >> 4, lc = lane & 15;
  const int B = a.batch, D = a.latent, S = D / 4, LD = D + 4;
  const int a0 = blockIdx.x * MMD_ROWS;
  const uint32_t step = a.prior_gen ? (uint32_t)*a.prior_step : 0u;
  const bool imq = a.kind == VAE_MMD_IMQ;
  const float Dsig = 2.f * (float)D * a.latent_var;                 // imq: C; rbf: sigma
  const float wscale = imq ? 1.f / Dsig : 1.f / ((float)D * Dsig * (float)B * (float)B);

  // ---- row fragments (B operand of the first product): row a0+lc, dims kg*S + s, of z and prior
  const int row = a0 + lc;
  const bool row_ok = row < B;
  float zr[SMAX], pr[SMAX];
  float zn = 0.f, pn = 0.f;
#pragma unroll
  for (int s4 = 0; s4 < SMAX / 4; ++s4) {
    f32x4 zv = {0.f, 0.f, 0.f, 0.f}, pv = {0.f, 0.f, 0.f, 0.f};
    if (4 * s4 < S && row_ok) {
      const int v4 = (kg * S) / 4 + s4;
      zv = z_vec(a, row, v4);
      pv = prior_vec(a, row, v4, step);
      if (a.prior_gen && wave == 0) *reinterpret_cast<f32x4*>(a.prior + (long)row * D + 4 * v4) = pv;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      zr[4 * s4 + i] = zv[i]; pr[4 * s4 + i] = pv[i];
      zn = fmaf(zv[i], zv[i], zn); pn = fmaf(pv[i], pv[i], pn);
    }
  }
  zn += __shfl_xor(zn, 16); zn += __shfl_xor(zn, 32);               // |z_row|^2, |p_row|^2 on all 4 lanes
  pn += __shfl_xor(pn, 16); pn += __shfl_xor(pn, 32);

  f32x4 G[DMAX / 16];                              // gradient tile: lane l reg r = G[row 4kg+r][16nt+lc]
#pragma unroll
  for (int nt = 0; nt < DMAX / 16; ++nt) G[nt] = f32x4{0.f, 0.f, 0.f, 0.f};
  float racc = 0.f;                                // sum_c coef[row lc][c] over this lane's columns
  double s_pp = 0.0, s_zz = 0.0, s_pz = 0.0;

  const int ntile = (B + CT - 1) / CT;             // column tiles per set; a tile never straddles sets
  for (int t = 0; t < 2 * ntile; ++t) {
    const bool pcols = t >= ntile;
    const int c0 = (pcols ? t - ntile : t) * CT;
    __syncthreads();                               // previous tile fully consumed
    for (int v = tid; v < CT * (D / 4); v += NT) {
      const int j = v / (D / 4), v4 = v - j * (D / 4);
      f32x4 u = {0.f, 0.f, 0.f, 0.f};
      if (c0 + j < B) u = pcols ? prior_vec(a, c0 + j, v4, step) : z_vec(a, c0 + j, v4);
      *reinterpret_cast<f32x4*>(cols + j * LD + 4 * v4) = u;
    }
    __syncthreads();
    if (tid < CT) {                                // |col|^2; lane t starts at dim -3t: distinct banks
      float s2 = 0.f;
      int d = (D - (3 * tid) % D) % D;
      for (int e = 0; e < D; ++e) {
        const float u = cols[tid * LD + d];
        s2 = fmaf(u, u, s2);
        d = d + 1 == D ? 0 : d + 1;
      }
      cn[tid] = s2;
    }
    __syncthreads();

    // ---- T[col][row] = U_col . row, for the latent rows and (prior columns only) the prior rows
    const int j0 = wave * 16;
    f32x4 tz = {0.f, 0.f, 0.f, 0.f}, tp = {0.f, 0.f, 0.f, 0.f};
    const float* cf = cols + (j0 + lc) * LD + kg * S;
#pragma unroll
    for (int s4 = 0; s4 < SMAX / 4; ++s4) {
      if (4 * s4 < S) {
        const f32x4 c4 = *reinterpret_cast<const f32x4*>(cf + 4 * s4);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          tz = __builtin_amdgcn_mfma_f32_16x16x4f32(c4[i], zr[4 * s4 + i], tz, 0, 0, 0);
          if (pcols) tp = __builtin_amdgcn_mfma_f32_16x16x4f32(c4[i], pr[4 * s4 + i], tp, 0, 0, 0);
        }
      }
    }
    // ---- kernel values of this lane's 4 columns (j0 + 4kg + r) against row lc
    f32x4 coef;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int cj = c0 + j0 + 4 * kg + r;         // column index within its set
      const float c2 = cn[j0 + 4 * kg + r];
      const bool ok = row_ok && cj < B;
      const bool diag = cj == row;
      // latent row x this column
      float d2 = fmaxf((zn + c2) - 2.f * tz[r], 0.f);
      float kv, w;
      if (imq) { kv = Dsig / (MMD_IMQ_EPS + Dsig + d2); w = kv * kv * wscale; }
      else { kv = expf(-((d2 / (float)D) / Dsig)); w = kv * wscale; }
      // imq drops i == j from all three matrices (prior-vs-z too); rbf keeps every entry
      if (!ok || (imq && diag)) { kv = 0.f; w = 0.f; }
      if (pcols) s_pz += (double)kv; else s_zz += (double)kv;
      coef[r] = pcols ? -4.f * w : 4.f * w;
      if (pcols) {                                 // prior row x prior column
        d2 = fmaxf((pn + c2) - 2.f * tp[r], 0.f);
        kv = imq ? Dsig / (MMD_IMQ_EPS + Dsig + d2) : expf(-((d2 / (float)D) / Dsig));
        if (!ok || (imq && diag)) kv = 0.f;
        s_pp += (double)kv;
      }
    }
    racc += (coef[0] + coef[1]) + (coef[2] + coef[3]);
    // ---- G[row][n] += sum_j coef[j][row] U[j][n]: k-step r pairs coef[r] with column j0 + 4kg + r
#pragma unroll
    for (int nt = 0; nt < DMAX / 16; ++nt) {
      if (16 * nt < D) {
#pragma unroll
        for (int r = 0; r < 4; ++r)
          G[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(coef[r], cols[(j0 + 4 * kg + r) * LD + 16 * nt + lc], G[nt], 0, 0, 0);
      }
    }
  }

  // ---- combine the waves: sums (double), coefficient row sums, gradient tiles
  for (int off = 32; off > 0; off >>= 1) {
    s_pp += __shfl_xor(s_pp, off); s_zz += __shfl_xor(s_zz, off); s_pz += __shfl_xor(s_pz, off);
  }
  racc += __shfl_xor(racc, 16); racc += __shfl_xor(racc, 32);
  __syncthreads();                                 // last tile consumed: cols becomes G[NW][16][D]
  if (lane == 0) { sums[wave][0] = s_pp; sums[wave][1] = s_zz; sums[wave][2] = s_pz; }
  if (kg == 0) rs[wave][lc] = racc;
#pragma unroll
  for (int nt = 0; nt < DMAX / 16; ++nt) {
    if (16 * nt < D) {
#pragma unroll
      for (int r = 0; r < 4; ++r) cols[(wave * 16 + 4 * kg + r) * D + 16 * nt + lc] = G[nt][r];
    }
  }
  __syncthreads();
  if (tid == 0) {
    double pp = 0.0, zz = 0.0, pz = 0.0;
    for (int w = 0; w < NW; ++w) { pp += sums[w][0]; zz += sums[w][1]; pz += sums[w][2]; }
    const double nrm = imq ? 1.0 : 1.0 / ((double)B * (double)B);
    double* o = k.partials + 4 * blockIdx.x;
    o[0] = pp * nrm; o[1] = zz * nrm; o[2] = pz * nrm; o[3] = 0.0;
  }
  for (int v = tid; v < MMD_ROWS * D; v += NT) {
    const int ar = v / D, d = v - ar * D;
    const int gr = a0 + ar;
    if (gr >= B) continue;
    float g = 0.f, r = 0.f;
    for (int w = 0; w < NW; ++w) { g += cols[(w * 16 + ar) * D + d]; r += rs[w][ar]; }
    const float mu = a.mulv[(long)gr * 2 * D + d], lv = a.mulv[(long)gr * 2 * D + D + d];
    const float e = a.eps[(long)gr * D + d];
    const float sd = expf(0.5f * lv);
    const float z = fmaf(e, sd, mu);
    const float dz = a.grad_scale * (g - r * z);
    a.dz[(long)gr * D + d] = dz;
    if (a.dmulv) {                                 // one thread owns each element: plain adds
      a.dmulv[(long)gr * 2 * D + d] += dz;
      a.dmulv[(long)gr * 2 * D + D + d] += dz * 0.5f * e * sd;
    }
  }
}

__global__ void __launch_bounds__(256) mmd_reseed_kernel(int n, int D, const float* dz, const float* scale,
                                                         const float* mulv, const float* eps, float* dmulv) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int b = i / D, d = i - b * D;
  const float g = *scale * dz[i];
  const float sd = expf(0.5f * mulv[(long)b * 2 * D + D + d]);
  dmulv[(long)b * 2 * D + d] += g;
  dmulv[(long)b * 2 * D + D + d] += g * 0.5f * eps[i] * sd;
}

int mmd_check(const vae_mmd_args* a, const char* what) {
  if (!a) return fail(VAE_E_BADARG, "%s: null args", what);
  if (a->kind != VAE_MMD_IMQ && a->kind != VAE_MMD_RBF) return fail(VAE_E_BADARG, "%s: kernel kind %d", what, a->kind);
  if (a->batch < 2 || a->batch > 1024)
    return fail(VAE_E_BADSHAPE, "%s: batch %d (2 .. 1024; the reference divides by B(B-1))", what, a->batch);
  if (a->latent <= 0 || a->latent % 32 || a->latent > 256)
    return fail(VAE_E_BADSHAPE, "%s: latent %d (a multiple of 32, <= 256)", what, a->latent);
  if (!(a->latent_var > 0.f)) return fail(VAE_E_BADARG, "%s: latent_var %g", what, (double)a->latent_var);
  return VAE_OK;
}

inline bool al16p(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace
}  // namespace vae

using namespace vae;

extern "C" int vae_mmd_workspace_size(const vae_mmd_args* a, size_t* bytes, int32_t* tiles) {
  if (!bytes) return fail(VAE_E_BADARG, "mmd_workspace_size: null argument");
  if (int rc = mmd_check(a, "mmd_workspace_size")) return rc;
  const int nt = (a->batch + MMD_ROWS - 1) / MMD_ROWS;
  *bytes = (size_t)nt * 4 * sizeof(double);
  if (tiles) *tiles = nt;
  return VAE_OK;
}

extern "C" int vae_mmd_fwd(const vae_mmd_args* a, void* stream) {
  if (int rc = mmd_check(a, "mmd_fwd")) return rc;
  if (!a->mulv || !a->eps || !a->prior || !a->dz || !a->workspace) return fail(VAE_E_BADARG, "mmd_fwd: mulv / eps / prior / dz / workspace");
  if (!al16p(a->mulv) || !al16p(a->eps) || !al16p(a->prior) || (reinterpret_cast<uintptr_t>(a->workspace) & 7))
    return fail(VAE_E_BADARG, "mmd_fwd: mulv / eps / prior must be 16-byte aligned, the workspace 8");
  if (a->prior_gen && !a->prior_step) return fail(VAE_E_BADARG, "mmd_fwd: prior_gen needs prior_step");
  const int nt = (a->batch + MMD_ROWS - 1) / MMD_ROWS;
  if (a->workspace_bytes < (int64_t)nt * 4 * (int64_t)sizeof(double))
    return fail(VAE_E_BADARG, "mmd_fwd: workspace of %ld bytes < %ld required (see vae_mmd_workspace_size)",
                (long)a->workspace_bytes, (long)nt * 4 * (long)sizeof(double));
  MmdK k{*a, static_cast<double*>(a->workspace)};
  hipStream_t st = (hipStream_t)stream;
  if (a->latent <= 128) VAE_LAUNCH((mmd_kernel<128, 4>), dim3(nt), dim3(256), 0, st, k);
  else VAE_LAUNCH((mmd_kernel<256, 2>), dim3(nt), dim3(128), 0, st, k);
  return check_launch("mmd_fwd");
}

extern "C" int vae_mmd_reseed(int32_t batch, int32_t latent, const float* dz, const float* scale, const float* mulv,
                              const float* eps, float* dmulv, void* stream) {
  if (!dz || !scale || !mulv || !eps || !dmulv) return fail(VAE_E_BADARG, "mmd_reseed: null tensor");
  if (batch <= 0 || latent <= 0 || (long)batch * latent >= (1l << 31)) return fail(VAE_E_BADSHAPE, "mmd_reseed: sizes");
  const int n = batch * latent;
  VAE_LAUNCH(mmd_reseed_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, n, latent, dz, scale, mulv,
             eps, dmulv);
  return check_launch("mmd_reseed");
}
