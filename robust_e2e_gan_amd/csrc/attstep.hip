// K7b: the content-based and coverage attention steps (AttDot, AttAdd, AttCov of model/e2e_attention.py) and their backward.
//
//   w = softmax_t( 2 * e[b,t] )      over ALL T frames incl. padding, as K7 (attloc.hip)
//   c = sum_t w[t] * enc[b,t]
//   add      : e = gvec . tanh(pre[b,t] + W_dec z[b]) + gb
//   coverage : e = gvec . tanh(wvec_w cov[b,t] + wvec_b + pre[b,t] + W_dec z[b]) + gb,   cov_{i+1} = cov_i + w_i,
//              cov_0[b,t] = 1/hlen_b for t < hlen_b, else 0 (a NULL cov_in stands for it)
//   dot      : e = sum_a pre[b,t,a] * q[b,a],  q = tanh(W_dec z[b] + b_dec);   pre = tanh(mlp_enc(enc)) is the caller's
// coverage_location is K7 itself with cov as att_prev (re2e_attloc_fwd / _bwd / _dpre); only its cov_{i+1} = cov_i + w_i is here
// (re2e_attstep_cov_add).
//
// The decomposition is K7's: a step is latency-bound, so the energies are cut into workgroups of 32 frames (grid = frame-chunks x
// utterances) and the parts that need all frames run once per utterance:
//   forward : attstep_decproj (A/64 x b)   -> dp[b,:] = W_dec z[b]   (dot: q[b,:])
//             attstep_energy (chunk x b)   -> e[b,t]
//             attstep_context (E/64 x b)   -> softmax over T, w[b,:], c[b, 64-column slice], cov_out = cov_in + w
//   backward: attstep_bwd_frames (chunk x b): de[t] = 2 w[t] (dw_in[t] + dc . enc[t] - s) with s = w . dw_in + dc . c (the forward
//             context is saved: no cross-workgroup reduction), d cov[t] = sum_a du[t][a] wvec_w[a], and the chunk's slab
//             sum_t du[t][a] (dot: sum_t de[t] pre[t][a]) of the d dec_proj sum
//             attstep_bwd_reduce (b): fixed-order sum of the chunk slabs -> d dec_proj (dot: times 1 - q^2)
//   after the loop: attstep_dpre (chunk16 x b): d_pre = sum_i du_i and the weight-gradient sums (gvec, gvec_b, wvec_w, wvec_b), per
//             chunk, then summed per utterance in fixed order; d_enc is K7's kind-independent re2e_attloc_denc.
// with du[t][a] = de[t] gvec[a] (1 - tanh^2(x[t][a])).  Wavefront shuffles do the reductions over the attention dimension, pre / enc rows
// are read row-contiguous (enc as float4).
//
// Limits (refused through re2e_last_error): adim <= 320 (five 64-lane slices held in registers), dunits <= 1024 (z in LDS), eprojs % 4 == 0,
// and eprojs / T such that the LDS tiles of the backward / the context pass fit (64 KiB / 160 KiB).
#include "common.h"

namespace {
constexpr int TCH = 32;        // frames per workgroup
constexpr int NTH = 256;       // threads per workgroup (4 wavefronts)
constexpr int NWV = NTH / 64;
constexpr int FPW = TCH / NWV; // frames per wavefront
constexpr int AIMAX = 5;       // max ceil(adim/64)
constexpr int TCD = 16;        // frames per workgroup of attstep_dpre
constexpr int DMAX = 1024;     // max dunits
constexpr int K_DOT = RE2E_ATT_DOT, K_ADD = RE2E_ATT_ADD, K_COV = RE2E_ATT_COVERAGE;

__device__ __forceinline__ float cov0(int t, int hl) { return t < hl ? 1.0f / (float)hl : 0.f; }

// dp[b][a] = sum_d W_dec[a][d] z[b][d]  (dot: tanh(. + b_dec[a])).  grid (ceil(A/64), B); 64 outputs x 4 slices of d per workgroup
__global__ __launch_bounds__(NTH) void attstep_decproj_kernel(const float* __restrict__ z, const float* __restrict__ w_decT,
                                                              const float* __restrict__ dec_b, int D, int A, float* __restrict__ dp_out) {
  __shared__ float zs[DMAX];
  __shared__ float part[4][64];
  const int b = blockIdx.y, a = blockIdx.x * 64 + (threadIdx.x & 63), dq = threadIdx.x >> 6;
  for (int d = threadIdx.x; d < D; d += NTH) zs[d] = z ? z[(long)b * D + d] : 0.f;
  __syncthreads();
  const int per = (D + 3) / 4, d0 = dq * per, d1 = min(D, d0 + per);
  float s0 = 0.f, s1 = 0.f;
  if (a < A) {
    int d = d0;
    for (; d + 16 <= d1; d += 16) {
      float w[16];
#pragma unroll
      for (int u = 0; u < 16; ++u) w[u] = w_decT[(long)(d + u) * A + a];
#pragma unroll
      for (int u = 0; u < 16; u += 2) { s0 += w[u] * zs[d + u]; s1 += w[u + 1] * zs[d + u + 1]; }
    }
    for (; d < d1; ++d) s0 += w_decT[(long)d * A + a] * zs[d];
  }
  part[dq][threadIdx.x & 63] = s0 + s1;
  __syncthreads();
  if (dq == 0 && a < A) {
    const float s = (part[0][threadIdx.x] + part[1][threadIdx.x]) + (part[2][threadIdx.x] + part[3][threadIdx.x]);
    dp_out[(long)b * A + a] = dec_b ? tanhf_(s + dec_b[a]) : s;
  }
}

// energies of one chunk of frames: a wavefront takes its 8 frames one after the other, lanes over the attention dimension.
// utt == nullptr: row b is utterance b with all T frames.  With a row -> utterance map row b reads pre[utt[b]] and HAS only
// Tr = hlens[utt[b]] frames (T is the pitch), as attloc_energy_kernel
template <int KIND>
__global__ __launch_bounds__(NTH) void attstep_energy_kernel(const float* __restrict__ pre, const float* __restrict__ dp_in,
                                                             const float* __restrict__ cov_in, const int* __restrict__ hlens,
                                                             const float* __restrict__ wvec_w, const float* __restrict__ wvec_b,
                                                             const float* __restrict__ gvec, const float* __restrict__ gvec_b, int T, int A,
                                                             float* __restrict__ e_out, const int* __restrict__ utt, int U) {
  const int b = blockIdx.y, t0 = blockIdx.x * TCH;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int u = utt ? min(max(utt[b], 0), U - 1) : b;
  const int hl = hlens[u];
  const int Tr = utt ? min(max(hl, 1), T) : T;
  const int nt = min(TCH, Tr - t0);
  if (nt <= 0) return;                                  // (uniform over the workgroup)
  float pv[FPW][AIMAX];
#pragma unroll
  for (int k = 0; k < FPW; ++k) {
    const int l = wid + NWV * k;
    const float* pr = pre + ((long)u * T + t0 + (l < nt ? l : 0)) * A;
#pragma unroll
    for (int i = 0; i < AIMAX; ++i) { int a = lane + 64 * i; pv[k][i] = a < A ? pr[a] : 0.f; }
  }
  float gv[AIMAX], dpv[AIMAX], ww[AIMAX], wb[AIMAX];
#pragma unroll
  for (int i = 0; i < AIMAX; ++i) {
    int a = lane + 64 * i;
    dpv[i] = a < A ? dp_in[(long)b * A + a] : 0.f;
    gv[i] = (KIND != K_DOT && a < A) ? gvec[a] : 0.f;
    ww[i] = (KIND == K_COV && a < A) ? wvec_w[a] : 0.f;
    wb[i] = (KIND == K_COV && a < A) ? wvec_b[a] : 0.f;
  }
  const float gb = KIND != K_DOT ? gvec_b[0] : 0.f;
#pragma unroll
  for (int k = 0; k < FPW; ++k) {
    const int l = wid + NWV * k;
    if (l >= nt) continue;                              // (uniform over the wavefront)
    const int t = t0 + l;
    float cv = 0.f;
    if (KIND == K_COV) cv = cov_in ? cov_in[(long)b * T + t] : cov0(t, hl);
    float sv = 0.f;
#pragma unroll
    for (int i = 0; i < AIMAX; ++i) {
      if (KIND == K_DOT) sv += pv[k][i] * dpv[i];       // (both 0 beyond A)
      else if (KIND == K_ADD) sv += gv[i] * tanhf_(pv[k][i] + dpv[i]);
      else sv += gv[i] * tanhf_((ww[i] * cv + wb[i]) + pv[k][i] + dpv[i]);
    }
    sv = wave_sum(sv);
    if (lane == 0) e_out[(long)b * T + t] = sv + gb;
  }
}

// softmax over the row's frames (recomputed per workgroup) + context for a 64-column slice (attloc_context_kernel) + the coverage carry
__global__ __launch_bounds__(NTH) void attstep_context_kernel(const float* __restrict__ e, const float* __restrict__ enc, int Tp, int E,
                                                              float* __restrict__ w_out, float* __restrict__ c_out, long ldc_out,
                                                              const float* __restrict__ cov_in, float* __restrict__ cov_out,
                                                              const int* __restrict__ utt, const int* __restrict__ hlens, int U) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  float* w = sm;                         // [Tp]
  float* red = w + ((Tp + 3) & ~3);      // [32]
  float* scr = red + 32;                 // [16][64]
  const int b = blockIdx.y, d0 = blockIdx.x * 64;
  const int tid = threadIdx.x;
  const int u = utt ? min(max(utt[b], 0), U - 1) : b;
  const int hl = hlens[u];
  const int T = utt ? min(max(hl, 1), Tp) : Tp;
  float m = -3.0e38f;
  for (int t = tid; t < T; t += NTH) { float v = 2.f * e[(long)b * Tp + t]; w[t] = v; m = fmaxf(m, v); }
  m = block_max(m, red);
  float sum = 0.f;
  for (int t = tid; t < T; t += NTH) { float v = __expf(w[t] - m); w[t] = v; sum += v; }
  sum = block_sum(sum, red);
  const float inv = 1.0f / sum;
  __syncthreads();
  for (int t = tid; t < T; t += NTH) {
    float v = w[t] * inv;
    w[t] = v;
    if (blockIdx.x == 0) {
      w_out[(long)b * Tp + t] = v;
      if (cov_out) cov_out[(long)b * Tp + t] = (cov_in ? cov_in[(long)b * Tp + t] : cov0(t, hl)) + v;
    }
  }
  if (blockIdx.x == 0)
    for (int t = T + tid; t < Tp; t += NTH) {
      w_out[(long)b * Tp + t] = 0.f;
      if (cov_out) cov_out[(long)b * Tp + t] = 0.f;
    }
  __syncthreads();
  // 16 float4 columns x 16 frame groups
  const int c4 = tid & 15, tg = tid >> 4;
  const int ncol = min(64, E - d0);
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  if (c4 * 4 < ncol) {
    const f32x4* er = reinterpret_cast<const f32x4*>(enc + (long)u * Tp * E + d0) + c4;
    const int per = E / 4;
    int t = tg;
    for (; t + 48 < T; t += 64) {
      f32x4 v0 = er[(long)t * per], v1 = er[(long)(t + 16) * per], v2 = er[(long)(t + 32) * per], v3 = er[(long)(t + 48) * per];
      acc += v0 * w[t] + v1 * w[t + 16] + v2 * w[t + 32] + v3 * w[t + 48];
    }
    for (; t < T; t += 16) acc += er[(long)t * per] * w[t];
  }
  *reinterpret_cast<f32x4*>(scr + tg * 64 + c4 * 4) = acc;
  __syncthreads();
  if (tid < ncol) {
    float s = 0.f;
#pragma unroll
    for (int g = 0; g < 16; ++g) s += scr[g * 64 + tid];
    c_out[(long)b * ldc_out + d0 + tid] = s;
  }
}

// cov_out = cov_in + w over (rows, T); cov_in == nullptr: cov_0 of the row's utterance
__global__ void attstep_cov_add_kernel(const float* __restrict__ cov_in, const float* __restrict__ w, const int* __restrict__ hlens,
                                       const int* __restrict__ utt, int U, int rows, int T, float* __restrict__ cov_out) {
  const long n = (long)rows * T;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    float c;
    if (cov_in) c = cov_in[i];
    else {
      const int b = (int)(i / T), t = (int)(i - (long)b * T);
      const int hl = hlens[utt ? min(max(utt[b], 0), U - 1) : b];
      c = cov0(t, hl);
    }
    cov_out[i] = c + w[i];
  }
}

// backward of one step for one chunk of frames: only what the recurrence needs (de, d cov, the d dec_proj slab)
template <int KIND>
__global__ __launch_bounds__(NTH) void attstep_bwd_frames_kernel(
    const float* __restrict__ pre, const float* __restrict__ enc, const float* __restrict__ w_cur, const float* __restrict__ dw_in,
    const float* __restrict__ dc, long ld_dc, const float* __restrict__ cx, const float* __restrict__ cov_in, const int* __restrict__ hlens,
    const float* __restrict__ dp_in, const float* __restrict__ wvec_w, const float* __restrict__ wvec_b, const float* __restrict__ gvec, int T,
    int E, int A, float* __restrict__ de_out, float* __restrict__ d_cov, float* __restrict__ slabs) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  float* dcs = sm;                              // [E]
  float* de = dcs + ((E + 3) & ~3);             // [TCH]
  float* red = de + TCH;                        // [32]
  float* wsl = red + 32;                        // [NWV][A]  per-wavefront slab parts
  const int b = blockIdx.y, chunk = blockIdx.x, t0 = chunk * TCH;
  const int nt = min(TCH, T - t0);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  // pre rows of this wavefront's frames: in flight while the softmax terms are computed
  float pv[FPW][AIMAX];
#pragma unroll
  for (int k = 0; k < FPW; ++k) {
    const int l = wid + NWV * k;
    const float* pr = pre + ((long)b * T + t0 + (l < nt ? l : 0)) * A;
#pragma unroll
    for (int i = 0; i < AIMAX; ++i) { int a = lane + 64 * i; pv[k][i] = a < A ? pr[a] : 0.f; }
  }
  // softmax normaliser  s = sum_t w[t] dw[t] = w . dw_in + dc . c
  float part = 0.f;
  for (int d = tid; d < E; d += NTH) { float g = dc[(long)b * ld_dc + d]; dcs[d] = g; part += g * cx[(long)b * E + d]; }
  if (dw_in)
    for (int t = tid; t < T; t += NTH) part += w_cur[(long)b * T + t] * dw_in[(long)b * T + t];
  const float sdot = block_sum(part, red);     // (contains the __syncthreads that publish dcs)
  // de[t] = 2 w[t] (dw_in[t] + dc . enc[t] - s): a wavefront takes four of its frames at a time
  const int per = E / 4;
#pragma unroll
  for (int k0 = 0; k0 < FPW; k0 += 4) {
    float sacc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int d4 = lane; d4 < per; d4 += 64) {
      f32x4 v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int l = wid + NWV * (k0 + u);
        v[u] = reinterpret_cast<const f32x4*>(enc + ((long)b * T + t0 + (l < nt ? l : 0)) * E)[d4];
      }
      const f32x4 g = *reinterpret_cast<const f32x4*>(dcs + d4 * 4);
#pragma unroll
      for (int u = 0; u < 4; ++u) sacc[u] += v[u][0] * g[0] + v[u][1] * g[1] + v[u][2] * g[2] + v[u][3] * g[3];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int l = wid + NWV * (k0 + u);
      const float sv = wave_sum(sacc[u]);
      if (lane == 0 && l < nt) {
        const long i0 = (long)b * T + t0 + l;
        const float v = 2.f * w_cur[i0] * (sv + (dw_in ? dw_in[i0] : 0.f) - sdot);
        de[l] = v;
        de_out[i0] = v;
      }
    }
  }
  __syncthreads();
  float gv[AIMAX], dpv[AIMAX], ww[AIMAX], wb[AIMAX], acc[AIMAX];
#pragma unroll
  for (int i = 0; i < AIMAX; ++i) {
    int a = lane + 64 * i;
    acc[i] = 0.f;
    dpv[i] = (KIND != K_DOT && a < A) ? dp_in[(long)b * A + a] : 0.f;
    gv[i] = (KIND != K_DOT && a < A) ? gvec[a] : 0.f;
    ww[i] = (KIND == K_COV && a < A) ? wvec_w[a] : 0.f;
    wb[i] = (KIND == K_COV && a < A) ? wvec_b[a] : 0.f;
  }
  const int hl = KIND == K_COV ? hlens[b] : 0;
#pragma unroll
  for (int k = 0; k < FPW; ++k) {
    const int l = wid + NWV * k;
    if (l >= nt) continue;                              // (uniform over the wavefront)
    const float det = de[l];
    const int t = t0 + l;
    float cv = 0.f, dcv = 0.f;
    if (KIND == K_COV) cv = cov_in ? cov_in[(long)b * T + t] : cov0(t, hl);
#pragma unroll
    for (int i = 0; i < AIMAX; ++i) {
      if (KIND == K_DOT) acc[i] += det * pv[k][i];
      else {
        const float x = KIND == K_COV ? (ww[i] * cv + wb[i]) + pv[k][i] + dpv[i] : pv[k][i] + dpv[i];
        const float u = tanhf_(x);
        const float d = det * gv[i] * (1.f - u * u);    // (gv is 0 beyond A)
        acc[i] += d;
        dcv += d * ww[i];
      }
    }
    if (KIND == K_COV && d_cov) {
      dcv = wave_sum(dcv);
      if (lane == 0) d_cov[(long)b * T + t] = dcv;
    }
  }
#pragma unroll
  for (int i = 0; i < AIMAX; ++i) { int a = lane + 64 * i; if (a < A) wsl[wid * A + a] = acc[i]; }
  __syncthreads();
  float* slab = slabs + ((long)b * gridDim.x + chunk) * A;
  for (int a = tid; a < A; a += NTH) slab[a] = (wsl[a] + wsl[A + a]) + (wsl[2 * A + a] + wsl[3 * A + a]);
}

// d dec_proj[b][a] = fixed-order sum of the chunk slabs (dot: times 1 - q^2, the gradient at the argument of the tanh)
__global__ __launch_bounds__(NTH) void attstep_bwd_reduce_kernel(const float* __restrict__ slabs, int nchunk, int A, const float* __restrict__ q,
                                                                 float* __restrict__ d_decproj) {
  const int b = blockIdx.x;
  const float* sl = slabs + (long)b * nchunk * A;
  for (int i = threadIdx.x; i < A; i += NTH) {
    float s = 0.f;
    for (int k = 0; k < nchunk; ++k) s += sl[(long)k * A + i];
    if (q) { const float v = q[(long)b * A + i]; s *= 1.f - v * v; }
    d_decproj[(long)b * A + i] = s;
  }
}

// after the decoder loop, for ALL steps at once: d_pre[b,t,a] = sum_i du_i[t][a] (dot: sum_i de_i[t] q_i[a]) and the chunk slab
//   [ dgvec(A) = sum de_i[t] tanh(x_i) | dwvec_w(A) = sum du_i cov_i[t] | dwvec_b(A) = sum du_i | dgb = sum de_i[t] ]
// (add: dgvec and dgb only, dot: none).  cov_all (L1,B,T) holds cov_{i+1} at step i, as the forward wrote it: step s reads
// cov_all[s-1], step 0 cov_0.  Thread = one attention unit a, all TCD frames in registers.
__host__ __device__ __forceinline__ int dpre_slab_floats(int kind, int A) { return kind == RE2E_ATT_COVERAGE ? 3 * A + 1 : kind == RE2E_ATT_ADD ? A + 1 : 0; }

template <int KIND>
__global__ __launch_bounds__(64 * AIMAX) void attstep_dpre_kernel(const float* __restrict__ pre, const float* __restrict__ cov_all,
                                                                  const int* __restrict__ hlens, const float* __restrict__ dp_all,
                                                                  const float* __restrict__ de_all, const float* __restrict__ wvec_w,
                                                                  const float* __restrict__ wvec_b, const float* __restrict__ gvec, int L1, int B,
                                                                  int T, int A, float* __restrict__ d_pre, float* __restrict__ slabs) {
  __shared__ float des[TCD];
  __shared__ float cvs[TCD];
  const int b = blockIdx.y, chunk = blockIdx.x, t0 = chunk * TCD;
  const int nt = min(TCD, T - t0);
  const int tid = threadIdx.x;
  const int a = tid;
  const bool on = a < A;
  float pv[TCD], acc[TCD];
#pragma unroll
  for (int l = 0; l < TCD; ++l) {
    pv[l] = (KIND != K_DOT && on && l < nt) ? pre[((long)b * T + t0 + l) * A + a] : 0.f;
    acc[l] = 0.f;
  }
  const float gv = (KIND != K_DOT && on) ? gvec[a] : 0.f;
  const float ww = (KIND == K_COV && on) ? wvec_w[a] : 0.f;
  const float wb = (KIND == K_COV && on) ? wvec_b[a] : 0.f;
  const int hl = KIND == K_COV ? hlens[b] : 0;
  float dgv = 0.f, dgb = 0.f, dww = 0.f, dwb = 0.f;
  for (int s = 0; s < L1; ++s) {
    const float dpv = on ? dp_all[((long)s * B + b) * A + a] : 0.f;
    __syncthreads();
    if (tid < TCD) {
      des[tid] = tid < nt ? de_all[((long)s * B + b) * T + t0 + tid] : 0.f;
      if (KIND == K_COV) cvs[tid] = tid < nt ? (s > 0 ? cov_all[((long)(s - 1) * B + b) * T + t0 + tid] : cov0(t0 + tid, hl)) : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int l = 0; l < TCD; ++l) {
      const float det = des[l];                   // 0 beyond the last frame
      if (KIND == K_DOT) acc[l] += det * dpv;
      else {
        const float cv = KIND == K_COV ? cvs[l] : 0.f;
        const float x = KIND == K_COV ? (ww * cv + wb) + pv[l] + dpv : pv[l] + dpv;
        const float u = tanhf_(x);
        const float d = det * gv * (1.f - u * u);
        acc[l] += d;
        dgv += det * u;
        dgb += det;
        dww += d * cv;
        dwb += d;
      }
    }
  }
  if (on) {
#pragma unroll
    for (int l = 0; l < TCD; ++l)
      if (l < nt) d_pre[((long)b * T + t0 + l) * A + a] = acc[l];
  }
  if (KIND != K_DOT) {
    float* slab = slabs + ((long)b * gridDim.x + chunk) * dpre_slab_floats(KIND, A);
    if (on) {
      slab[a] = dgv;
      if (KIND == K_COV) { slab[A + a] = dww; slab[2 * A + a] = dwb; }
    }
    if (tid == 0) slab[dpre_slab_floats(KIND, A) - 1] = dgb;
  }
}

// partials[b][gvec(A) | gvec_b(1) | wvec_w(A) | wvec_b(A)] += fixed-order sum of the chunk slabs of attstep_dpre
__global__ __launch_bounds__(NTH) void attstep_dpre_reduce_kernel(const float* __restrict__ slabs, int nchunk, int A, int SF, float* partials) {
  const int b = blockIdx.x;
  const float* sl = slabs + (long)b * nchunk * SF;
  float* part = partials + (long)b * SF;
  for (int i = threadIdx.x; i < SF; i += NTH) {
    float s = 0.f;
    for (int k = 0; k < nchunk; ++k) s += sl[(long)k * SF + i];
    if (i < A) part[i] += s;                  // gvec
    else if (i == SF - 1) part[A] += s;       // gvec_b
    else part[i + 1] += s;                    // wvec_w, wvec_b
  }
}

inline int nchunks(int T) { return (T + TCH - 1) / TCH; }
inline bool own_kind(int kind) { return kind == K_DOT || kind == K_ADD || kind == K_COV; }
}  // namespace

static int check_kind(const char* fn, int kind) {
  if (own_kind(kind)) return RE2E_OK;
  if (kind == RE2E_ATT_LOCATION || kind == RE2E_ATT_COVERAGE_LOCATION) {
    re2e_set_error("%s: attention kind %d (location / coverage_location) runs the re2e_attloc_* entry points, with cov as att_prev", fn, kind);
    return RE2E_EUNSUPPORTED;
  }
  re2e_set_error("%s: unknown attention kind %d", fn, kind);
  return RE2E_EINVAL;
}

static int check_dims(const char* fn, int B, int T, int E, int D, int A) {
  if (!(B > 0 && T > 0 && E > 0 && E % 4 == 0 && D > 0 && A > 0)) {
    re2e_set_error("%s: bad shape (B=%d T=%d eprojs=%d dunits=%d adim=%d; eprojs must be a multiple of 4)", fn, B, T, E, D, A);
    return RE2E_EINVAL;
  }
  if (A > 64 * AIMAX) { re2e_set_error("%s: adim <= %d supported (got %d)", fn, 64 * AIMAX, A); return RE2E_EUNSUPPORTED; }
  if (D > DMAX) { re2e_set_error("%s: dunits <= %d supported (got %d)", fn, DMAX, D); return RE2E_EUNSUPPORTED; }
  return RE2E_OK;
}

extern "C" size_t re2e_attstep_partial_floats(int kind, int adim) { return (size_t)dpre_slab_floats(kind, adim); }

extern "C" size_t re2e_attstep_workspace_bytes(int kind, int B, int T, int adim) {
  // per-step chunk slabs [B][nchunk][A] + attstep_dpre chunk slabs [B][ceil(T/16)][slab floats]
  return ((size_t)B * nchunks(T) * adim + (size_t)B * ((T + TCD - 1) / TCD) * dpre_slab_floats(kind, adim)) * sizeof(float);
}

// re2e_attstep_fwd (utt == nullptr: row b is utterance b, U = B) and re2e_attstep_fwd_rows: the same three launches
static int attstep_fwd_launch(const char* fn, int kind, const float* pre, const float* enc, const float* z, const float* cov_in, const int* hlens,
                              const int* utt, int U, const float* w_decT, const float* dec_b, const float* wvec_w, const float* wvec_b,
                              const float* gvec, const float* gvec_b, int B, int T, int E, int D, int A, float* w_out, float* c_out, long ldc_out,
                              float* cov_out, float* dp_out, float* e_scratch, hipStream_t stream) {
  int rc = check_kind(fn, kind);
  if (rc) return rc;
  rc = check_dims(fn, B, T, E, D, A);
  if (rc) return rc;
  if (kind == K_DOT ? !dec_b : !(gvec && gvec_b)) { re2e_set_error("%s: null parameter of attention kind %d", fn, kind); return RE2E_EINVAL; }
  if (kind == K_COV && !(wvec_w && wvec_b && cov_out)) { re2e_set_error("%s: coverage needs wvec and cov_out", fn); return RE2E_EINVAL; }
  const size_t lds2 = (size_t)(((T + 3) & ~3) + 32 + 16 * 64 + 16) * sizeof(float);
  if (lds2 > 160 * 1024) { re2e_set_error("%s: T=%d needs %zu bytes of LDS (>160 KiB)", fn, T, lds2); return RE2E_EUNSUPPORTED; }
  hipLaunchKernelGGL(attstep_decproj_kernel, dim3((A + 63) / 64, B), dim3(NTH), 0, stream, z, w_decT, kind == K_DOT ? dec_b : nullptr, D, A, dp_out);
  const dim3 g1(nchunks(T), B);
  if (kind == K_DOT)
    hipLaunchKernelGGL(attstep_energy_kernel<K_DOT>, g1, dim3(NTH), 0, stream, pre, (const float*)dp_out, cov_in, hlens, wvec_w, wvec_b, gvec, gvec_b, T, A,
                       e_scratch, utt, U);
  else if (kind == K_ADD)
    hipLaunchKernelGGL(attstep_energy_kernel<K_ADD>, g1, dim3(NTH), 0, stream, pre, (const float*)dp_out, cov_in, hlens, wvec_w, wvec_b, gvec, gvec_b, T, A,
                       e_scratch, utt, U);
  else
    hipLaunchKernelGGL(attstep_energy_kernel<K_COV>, g1, dim3(NTH), 0, stream, pre, (const float*)dp_out, cov_in, hlens, wvec_w, wvec_b, gvec, gvec_b, T, A,
                       e_scratch, utt, U);
  if (lds2 > 64 * 1024) (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&attstep_context_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds2);
  hipLaunchKernelGGL(attstep_context_kernel, dim3((E + 63) / 64, B), dim3(NTH), lds2, stream, (const float*)e_scratch, enc, T, E, w_out, c_out, ldc_out,
                     kind == K_COV ? cov_in : nullptr, kind == K_COV ? cov_out : nullptr, utt, hlens, U);
  hipError_t e__ = hipGetLastError();
  if (e__ != hipSuccess) { re2e_set_error("%s: launch failed: %s", fn, hipGetErrorString(e__)); return RE2E_EHIP; }
  return RE2E_OK;
}

extern "C" int re2e_attstep_fwd(int kind, const float* pre, const float* enc, const float* z, const float* cov_in, const int* hlens,
                                const float* w_decT, const float* dec_b, const float* wvec_w, const float* wvec_b, const float* gvec,
                                const float* gvec_b, int B, int T, int eprojs, int dunits, int adim, float* w_out, float* c_out, long ldc_out,
                                float* cov_out, float* dp_out, float* e_scratch, hipStream_t stream) {
  RE2E_CHECK_ARG(pre && enc && hlens && w_decT && w_out && c_out && dp_out && e_scratch, "null arg");
  return attstep_fwd_launch("re2e_attstep_fwd", kind, pre, enc, z, cov_in, hlens, nullptr, B, w_decT, dec_b, wvec_w, wvec_b, gvec, gvec_b, B, T, eprojs,
                            dunits, adim, w_out, c_out, ldc_out, cov_out, dp_out, e_scratch, stream);
}

extern "C" int re2e_attstep_fwd_rows(int kind, const float* pre, const float* enc, int U, const int* hlens, const int* utt_dev, const float* z,
                                     const float* cov_in, const float* w_decT, const float* dec_b, const float* wvec_w, const float* wvec_b,
                                     const float* gvec, const float* gvec_b, int nh, int T, int eprojs, int dunits, int adim, float* w_out,
                                     float* c_out, long ldc_out, float* cov_out, float* dp_out, float* e_scratch, hipStream_t stream) {
  RE2E_CHECK_ARG(pre && enc && hlens && utt_dev && w_decT && w_out && c_out && dp_out && e_scratch, "null arg");
  RE2E_CHECK_ARG(U > 0, "no utterances");
  return attstep_fwd_launch("re2e_attstep_fwd_rows", kind, pre, enc, z, cov_in, hlens, utt_dev, U, w_decT, dec_b, wvec_w, wvec_b, gvec, gvec_b, nh, T,
                            eprojs, dunits, adim, w_out, c_out, ldc_out, cov_out, dp_out, e_scratch, stream);
}

extern "C" int re2e_attstep_cov_add(const float* cov_in, const float* w, const int* hlens, const int* utt_dev, int U, int rows, int T,
                                    float* cov_out, hipStream_t stream) {
  RE2E_CHECK_ARG(w && hlens && cov_out && rows > 0 && T > 0 && U > 0, "bad args");
  const long n = (long)rows * T;
  hipLaunchKernelGGL(attstep_cov_add_kernel, dim3((unsigned)min((n + 255) / 256, (long)1024)), dim3(256), 0, stream, cov_in, w, hlens, utt_dev, U, rows, T,
                     cov_out);
  RE2E_LAUNCH_CHECK();
  return RE2E_OK;
}

extern "C" int re2e_attstep_bwd(int kind, const float* pre, const float* enc, const float* cov_in, const float* w_cur, const int* hlens,
                                const float* wvec_w, const float* wvec_b, const float* gvec, const float* dp_in, const float* cx_in,
                                const float* dc, long ld_dc, const float* dw_in, int B, int T, int eprojs, int adim, float* de_out, float* d_cov,
                                float* d_decproj, void* workspace, size_t workspace_bytes, hipStream_t stream) {
  RE2E_CHECK_ARG(pre && enc && w_cur && hlens && dp_in && cx_in && dc && de_out && d_decproj && workspace, "null arg");
  int rc = check_kind("re2e_attstep_bwd", kind);
  if (rc) return rc;
  rc = check_dims("re2e_attstep_bwd", B, T, eprojs, 1, adim);
  if (rc) return rc;
  RE2E_CHECK_ARG(kind == K_DOT || gvec, "null gvec");
  RE2E_CHECK_ARG(kind != K_COV || (wvec_w && wvec_b), "coverage needs wvec");
  RE2E_CHECK_ARG(workspace_bytes >= re2e_attstep_workspace_bytes(kind, B, T, adim), "workspace too small");
  const int nch = nchunks(T);
  float* slabs = (float*)workspace;
  const size_t lds = (size_t)(((eprojs + 3) & ~3) + TCH + 32 + NWV * adim + 16) * sizeof(float);
  if (lds > 64 * 1024) { re2e_set_error("re2e_attstep_bwd: eprojs=%d needs %zu bytes of LDS (>64 KiB)", eprojs, lds); return RE2E_EUNSUPPORTED; }
  const dim3 g(nch, B);
  if (kind == K_DOT)
    hipLaunchKernelGGL(attstep_bwd_frames_kernel<K_DOT>, g, dim3(NTH), lds, stream, pre, enc, w_cur, dw_in, dc, ld_dc, cx_in, cov_in, hlens, dp_in, wvec_w,
                       wvec_b, gvec, T, eprojs, adim, de_out, d_cov, slabs);
  else if (kind == K_ADD)
    hipLaunchKernelGGL(attstep_bwd_frames_kernel<K_ADD>, g, dim3(NTH), lds, stream, pre, enc, w_cur, dw_in, dc, ld_dc, cx_in, cov_in, hlens, dp_in, wvec_w,
                       wvec_b, gvec, T, eprojs, adim, de_out, d_cov, slabs);
  else
    hipLaunchKernelGGL(attstep_bwd_frames_kernel<K_COV>, g, dim3(NTH), lds, stream, pre, enc, w_cur, dw_in, dc, ld_dc, cx_in, cov_in, hlens, dp_in, wvec_w,
                       wvec_b, gvec, T, eprojs, adim, de_out, d_cov, slabs);
  hipLaunchKernelGGL(attstep_bwd_reduce_kernel, dim3(B), dim3(NTH), 0, stream, (const float*)slabs, nch, adim, kind == K_DOT ? dp_in : nullptr, d_decproj);
  RE2E_LAUNCH_CHECK();
  return RE2E_OK;
}

extern "C" int re2e_attstep_dpre(int kind, const float* pre, const float* cov_all, const int* hlens, const float* dp_all, const float* de_all,
                                 const float* wvec_w, const float* wvec_b, const float* gvec, int L1, int B, int T, int adim, float* d_pre,
                                 float* partials, void* workspace, size_t workspace_bytes, hipStream_t stream) {
  RE2E_CHECK_ARG(pre && hlens && dp_all && de_all && d_pre && workspace && L1 > 0, "bad args");
  int rc = check_kind("re2e_attstep_dpre", kind);
  if (rc) return rc;
  rc = check_dims("re2e_attstep_dpre", B, T, 4, 1, adim);
  if (rc) return rc;
  RE2E_CHECK_ARG(kind == K_DOT || (gvec && partials), "null gvec / partials");
  RE2E_CHECK_ARG(kind != K_COV || (wvec_w && wvec_b && (cov_all || L1 == 1)), "coverage needs wvec and the saved cov rows");
  RE2E_CHECK_ARG(workspace_bytes >= re2e_attstep_workspace_bytes(kind, B, T, adim), "workspace too small");
  const int nch = nchunks(T), ncd = (T + TCD - 1) / TCD;
  float* slabs = (float*)workspace + (size_t)B * nch * adim;
  const dim3 g(ncd, B), th(64 * ((adim + 63) / 64));
  if (kind == K_DOT)
    hipLaunchKernelGGL(attstep_dpre_kernel<K_DOT>, g, th, 0, stream, pre, cov_all, hlens, dp_all, de_all, wvec_w, wvec_b, gvec, L1, B, T, adim, d_pre, slabs);
  else if (kind == K_ADD)
    hipLaunchKernelGGL(attstep_dpre_kernel<K_ADD>, g, th, 0, stream, pre, cov_all, hlens, dp_all, de_all, wvec_w, wvec_b, gvec, L1, B, T, adim, d_pre, slabs);
  else
    hipLaunchKernelGGL(attstep_dpre_kernel<K_COV>, g, th, 0, stream, pre, cov_all, hlens, dp_all, de_all, wvec_w, wvec_b, gvec, L1, B, T, adim, d_pre, slabs);
  if (kind != K_DOT)
    hipLaunchKernelGGL(attstep_dpre_reduce_kernel, dim3(B), dim3(NTH), 0, stream, (const float*)slabs, ncd, adim, dpre_slab_floats(kind, adim), partials);
  RE2E_LAUNCH_CHECK();
  return RE2E_OK;
}
