// Upper layers of a multi-layer attention decoder (dlayers > 1, e2e_decoder.py:121-152): layer l >= 1 is a plain LSTMCell on the state of the
// layer below at the same token and on its own previous state.  The attention reads layer 0 only, so layer 0 keeps its loop (decloop.hip /
// attloc.hip / attstep.hip) and the layers above are a stacked LSTM over its output z0 (L1,B,D); they run per token only where a token is sampled
// from the top layer's output (scheduled sampling, the greedy attention dump, beam search).
//
// Every product here has B <= a few dozen rows (utterances, or utterances x beam) against a (4D,D) weight matrix of which a row is a hidden
// unit's gate: fp32 on the vector ALUs, one wavefront per hidden unit, the way csrc/rnnlm.hip runs the RNNLM's cell.  A wavefront reads the four
// gate rows of its unit straight into registers as float4 against 8 activation rows, reduces the 4 x 8 lane-partial sums with a transposing
// butterfly and applies the cell itself: no LDS, no barrier in the forward kernel.  The sum of a row does not depend on which other rows share
// its launch or on its place among them (per-lane fmaf chain in k order, then the same balanced tree over the lanes for every value), which the
// beam search relies on: a hypothesis scores the same in any batch.
//
//   upper_cell_kernel<false>   sequence step: gates[i] (input projection + both biases, made for all tokens by ONE re2e_gemm) += z[i] W_hh^T,
//                              then the cell -> activated gates, c[i+1], z[i+1]                       (re2e_dec_upper_seq_fwd: one launch per token)
//   upper_cell_kernel<true>    token step for n rows: gates = b_ih + b_hh + x W_ih^T + z_prev W_hh^T, then the cell  (re2e_dec_upper_step)
//   upper_bwd_kernel           cell backward of one token (dh = carried + dZ[i], dc) -> pre-activation d(gates)[i], dc_prev, and
//                              dz_prev = d(gates)[i] W_hh in the same launch                           (re2e_dec_upper_seq_bwd: one launch per token)
//
// re2e_dec_gates_cell_fwd (lstm.hip) was not reused for the token step: it wants the gates pre-filled with the biases (one more launch per
// layer and position) and its MFMA tile pads every launch to 32 rows.  No kernel here waits on another workgroup.
#include "common.h"

namespace {

constexpr int UR = 8;          // activation rows per workgroup
constexpr int UW = 4;          // wavefronts per workgroup = hidden units per workgroup (forward) = output units of dz_prev per workgroup (backward)

// Sum v[i] over the 64 lanes for all NV values at once (csrc/rnnlm.hip): every step halves the values a lane carries.  The total of value i
// ends in lanes i * (64 / NV) .. (i + 1) * (64 / NV) - 1; the tree over the lanes (32, 16, 8, 4, 2, 1) is the same for every i.
template <int CNT, int OFF, int NV>
__device__ __forceinline__ void reduce_step(float (&v)[NV], int lane) {
  if constexpr (CNT > 1) {
    constexpr int HALF = CNT / 2;
    const bool up = (lane & OFF) != 0;
#pragma unroll
    for (int i = 0; i < HALF; ++i) {
      const float keep = up ? v[i + HALF] : v[i];
      const float send = up ? v[i] : v[i + HALF];
      v[i] = keep + __shfl_xor(send, OFF, 64);
    }
    reduce_step<HALF, OFF / 2, NV>(v, lane);
  }
}
template <int NV>
__device__ __forceinline__ float reduce_transposed(float (&v)[NV], int lane) {
  static_assert(NV == 8 || NV == 16 || NV == 32, "values per lane");
  reduce_step<NV, 32, NV>(v, lane);
  float s = v[0];
#pragma unroll
  for (int o = 64 / NV / 2; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  return s;
}

// acc[g * UR + r] += sum_k w[g][k] * act[aoff[r] + k] over this lane's float4 pieces of k (K % 4 == 0)
__device__ __forceinline__ void dot_rows(const float* const (&w)[4], const float* __restrict__ act, const int (&aoff)[UR], int K, int lane,
                                         float (&acc)[4 * UR]) {
  for (int k = lane * 4; k < K; k += 256) {
    f32x4 wv[4], av[UR];
#pragma unroll
    for (int g = 0; g < 4; ++g) wv[g] = *reinterpret_cast<const f32x4*>(w[g] + k);
#pragma unroll
    for (int r = 0; r < UR; ++r) av[r] = *reinterpret_cast<const f32x4*>(act + aoff[r] + k);
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
      for (int r = 0; r < UR; ++r)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[g * UR + r] = fmaf(wv[g][e], av[r][e], acc[g * UR + r]);
  }
}

// One LSTMCell step of an upper layer (torch gate order i, f, g, o).  grid (ceil(D / UW), ceil(n / UR)); wavefront = hidden unit j.
// HAS_X: gates = b_ih + b_hh + x W_ih^T + z_prev W_hh^T (x (n,D)), `gates` (n,4D) optional output of the activated gates.
// !HAS_X: `gates` holds the input projection and both biases on entry, the activated gates on exit.
template <bool HAS_X>
__global__ __launch_bounds__(64 * UW) void upper_cell_kernel(const float* __restrict__ x, const float* __restrict__ w_ih, const float* __restrict__ b_ih,
                                                             const float* __restrict__ b_hh, const float* __restrict__ z_prev,
                                                             const float* __restrict__ w_hh, float* gates, const float* __restrict__ c_prev,
                                                             float* __restrict__ c_out, float* __restrict__ z_out, int n, int D) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int j = blockIdx.x * UW + wave;
  if (j >= D) return;                                       // (no barrier below)
  const int row0 = blockIdx.y * UR;
  const int nr = min(UR, n - row0);
  int aoff[UR];
#pragma unroll
  for (int r = 0; r < UR; ++r) aoff[r] = (row0 + (r < nr ? r : 0)) * D;      // rows beyond the batch alias the tile's first row; never stored
  const bool fin = lane < nr;                               // lane r finishes row row0 + r
  const long row = row0 + (fin ? lane : 0);
  const long o = row * D + j;
  const float cp = fin ? c_prev[o] : 0.f;
  float base[4];
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    if (HAS_X) base[g] = fin ? b_ih[g * D + j] + b_hh[g * D + j] : 0.f;
    else base[g] = fin ? gates[row * 4 * D + (long)g * D + j] : 0.f;
  }
  float acc[4 * UR];
#pragma unroll
  for (int i = 0; i < 4 * UR; ++i) acc[i] = 0.f;
  const float* wr[4];
  if (HAS_X) {
#pragma unroll
    for (int g = 0; g < 4; ++g) wr[g] = w_ih + ((long)g * D + j) * D;
    dot_rows(wr, x, aoff, D, lane, acc);
  }
#pragma unroll
  for (int g = 0; g < 4; ++g) wr[g] = w_hh + ((long)g * D + j) * D;
  dot_rows(wr, z_prev, aoff, D, lane, acc);
  const float s = reduce_transposed<4 * UR>(acc, lane);     // value g * UR + r in lanes 2 (g UR + r), 2 (g UR + r) + 1
  float v[4];
#pragma unroll
  for (int g = 0; g < 4; ++g) v[g] = __shfl(s, 2 * (g * UR + (lane & (UR - 1))), 64);
  if (fin) {
    const float gi = sigmoidf_(base[0] + v[0]), gf = sigmoidf_(base[1] + v[1]), gg = tanhf_(base[2] + v[2]), go = sigmoidf_(base[3] + v[3]);
    const float c = gf * cp + gi * gg;
    if (gates) {
      float* gp = gates + row * 4 * D + j;
      gp[0] = gi; gp[D] = gf; gp[2L * D] = gg; gp[3L * D] = go;
    }
    c_out[o] = c;
    z_out[o] = go * tanhf_(c);
  }
}

// One token of an upper layer's backward.  grid (ceil(D / UW), ceil(B / UR)), dynamic LDS UR x 4D floats.  Every workgroup of a row tile
// derives the tile's d(gates) (UR x 4D, element-wise: cheap beside the product, and the operands stay in L2) into LDS; the workgroups of
// column block 0 also store them (dG, pre-activation gradients: what the weight-gradient products read) and dc_prev.  Then wavefront w takes
// output unit blockIdx.x * UW + w: dz_prev[b][k] = sum_r dG[b][r] W_hh[r][k] with W_hh^T (D,4D) so that the contraction runs along a row.  (Sixteen units
// per workgroup, four per wavefront one after the other, recomputed less and measured slower: 0.23 ms per layer on the flagship loop's
// forward+backward, profiles/dlayers.md.)  dh, dc_in are read by every workgroup of the tile and dh_out, dc_out written by some: the caller
// alternates two buffers of each.
__global__ __launch_bounds__(64 * UW) void upper_bwd_kernel(const float* __restrict__ gates, const float* __restrict__ c_prev,
                                                            const float* __restrict__ c_cur, const float* __restrict__ dh,
                                                            const float* __restrict__ dz, const float* __restrict__ dc_in,
                                                            const float* __restrict__ w_hhT, float* __restrict__ dG, float* __restrict__ dc_out,
                                                            float* __restrict__ dh_out, int B, int D) {
  extern __shared__ float sdg[];                            // [UR][4D]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int row0 = blockIdx.y * UR, k = blockIdx.x * UW + wave;
  const int nr = min(UR, B - row0);
  const int D4 = 4 * D;
  const bool store = blockIdx.x == 0;
  for (int e = tid; e < UR * D; e += 64 * UW) {
    const int r = e / D, u = e - r * D;
    float d0 = 0.f, d1 = 0.f, d2 = 0.f, d3 = 0.f;
    if (r < nr) {
      const long i = (long)(row0 + r) * D + u;
      const float* g = gates + (long)(row0 + r) * D4 + u;
      const float gi = g[0], gf = g[D], gg = g[2L * D], go = g[3L * D];
      const float tc = tanhf_(c_cur[i]);
      const float d = dh[i] + dz[i];                        // recurrent + direct gradient of this token's state
      const float dct = d * go * (1.f - tc * tc) + dc_in[i];
      d0 = dct * gg * gi * (1.f - gi);
      d1 = dct * c_prev[i] * gf * (1.f - gf);
      d2 = dct * gi * (1.f - gg * gg);
      d3 = d * tc * go * (1.f - go);
      if (store) {
        float* o = dG + (long)(row0 + r) * D4 + u;
        o[0] = d0; o[D] = d1; o[2L * D] = d2; o[3L * D] = d3;
        dc_out[i] = dct * gf;
      }
    }
    float* s = sdg + r * D4 + u;                             // rows beyond the batch: zeros
    s[0] = d0; s[D] = d1; s[2 * D] = d2; s[3 * D] = d3;
  }
  __syncthreads();
  if (k < D) {                                              // (wave-uniform; no barrier below)
    const float* wr = w_hhT + (long)k * D4;
    float acc[UR];
#pragma unroll
    for (int r = 0; r < UR; ++r) acc[r] = 0.f;
#pragma unroll 4
    for (int c4 = lane * 4; c4 < D4; c4 += 256) {
      const f32x4 wv = *reinterpret_cast<const f32x4*>(wr + c4);
#pragma unroll
      for (int r = 0; r < UR; ++r) {
        const f32x4 sv = *reinterpret_cast<const f32x4*>(sdg + r * D4 + c4);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[r] = fmaf(wv[e], sv[e], acc[r]);
      }
    }
    const float s = reduce_transposed<UR>(acc, lane);       // row r in lanes 8 r .. 8 r + 7
    const int r = lane >> 3;
    if ((lane & 7) == 0 && r < nr) dh_out[(long)(row0 + r) * D + k] = s;
  }
}

LdsLimit g_bwd_lds;

bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// D % 4 == 0 and D <= 1024: rows are read as float4, and UR rows of d(gates) fit the backward's LDS (UR x 4D floats = 128 KiB at 1024)
int check_width(const char* fn, int D) {
  if (D % 4 != 0 || D > 1024) {
    re2e_set_error("%s: dunits must be a multiple of 4 and at most 1024 (got %d)", fn, D);
    return RE2E_EUNSUPPORTED;
  }
  return RE2E_OK;
}

}  // namespace

extern "C" int re2e_dec_upper_step(const float* x, const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh, const float* z_prev,
                                   const float* c_prev, float* gates, float* z_out, float* c_out, int n, int D, hipStream_t stream) {
  RE2E_CHECK_ARG(x && w_ih && w_hh && b_ih && b_hh && z_prev && c_prev && z_out && c_out, "null operand");
  RE2E_CHECK_ARG(n > 0 && D > 0, "bad shape");
  if (const int rc = check_width(__func__, D)) return rc;
  RE2E_CHECK_ARG((long)n * 4 * D < (1L << 31), "operand beyond 32-bit element offsets");
  RE2E_CHECK_ARG(al16(x) && al16(w_ih) && al16(w_hh) && al16(z_prev), "x, w_ih, w_hh, z_prev must be 16-byte aligned");
  RE2E_CHECK_ARG(z_out != z_prev && z_out != x && c_out != z_prev && c_out != x, "x and z_prev are read by every workgroup: the outputs must not alias them");
  hipLaunchKernelGGL(upper_cell_kernel<true>, dim3(cdiv(D, UW), cdiv(n, UR)), dim3(64 * UW), 0, stream, x, w_ih, b_ih, b_hh, z_prev, w_hh, gates, c_prev,
                     c_out, z_out, n, D);
  RE2E_LAUNCH_CHECK();
  return RE2E_OK;
}

extern "C" int re2e_dec_upper_seq_fwd(float* gates, const float* w_hh, float* z, float* c, int L1, int B, int D, hipStream_t stream) {
  RE2E_CHECK_ARG(gates && w_hh && z && c, "null operand");
  RE2E_CHECK_ARG(L1 > 0 && B > 0 && D > 0, "bad shape");
  if (const int rc = check_width(__func__, D)) return rc;
  RE2E_CHECK_ARG((long)B * 4 * D < (1L << 31), "operand beyond 32-bit element offsets");
  RE2E_CHECK_ARG(al16(w_hh) && al16(z), "w_hh and z must be 16-byte aligned");
  const long bd = (long)B * D;
  for (int i = 0; i < L1; ++i)
    hipLaunchKernelGGL(upper_cell_kernel<false>, dim3(cdiv(D, UW), cdiv(B, UR)), dim3(64 * UW), 0, stream, (const float*)nullptr, (const float*)nullptr,
                       (const float*)nullptr, (const float*)nullptr, (const float*)(z + i * bd), w_hh, gates + i * 4 * bd, (const float*)(c + i * bd),
                       c + (i + 1) * bd, z + (i + 1) * bd, B, D);
  RE2E_LAUNCH_CHECK();
  return RE2E_OK;
}

extern "C" size_t re2e_dec_upper_bwd_workspace_bytes(int B, int D) {
  return B > 0 && D > 0 ? (size_t)4 * B * D * sizeof(float) : 0;
}

extern "C" int re2e_dec_upper_seq_bwd(const float* gates, const float* c, const float* dZ, const float* w_hhT, float* dG, int L1, int B, int D,
                                      void* workspace, size_t workspace_bytes, hipStream_t stream) {
  RE2E_CHECK_ARG(gates && c && dZ && w_hhT && dG && workspace, "null operand");
  RE2E_CHECK_ARG(L1 > 0 && B > 0 && D > 0, "bad shape");
  if (const int rc = check_width(__func__, D)) return rc;
  RE2E_CHECK_ARG((long)B * 4 * D < (1L << 31), "operand beyond 32-bit element offsets");
  RE2E_CHECK_ARG(al16(w_hhT), "w_hhT must be 16-byte aligned");
  RE2E_CHECK_ARG(workspace_bytes >= re2e_dec_upper_bwd_workspace_bytes(B, D), "workspace too small (re2e_dec_upper_bwd_workspace_bytes)");
  const long bd = (long)B * D;
  float* dh[2] = {(float*)workspace, (float*)workspace + bd};
  float* dc[2] = {(float*)workspace + 2 * bd, (float*)workspace + 3 * bd};
  if (hipMemsetAsync(dh[0], 0, bd * sizeof(float), stream) != hipSuccess || hipMemsetAsync(dc[0], 0, bd * sizeof(float), stream) != hipSuccess) {
    re2e_set_error("%s: hipMemsetAsync failed", __func__);
    return RE2E_EHIP;
  }
  const size_t lds = (size_t)UR * 4 * D * sizeof(float);
  if (lds > 64 * 1024) g_bwd_lds.ensure(reinterpret_cast<const void*>(&upper_bwd_kernel), lds);
  int cur = 0;
  for (int i = L1 - 1; i >= 0; --i, cur ^= 1)
    hipLaunchKernelGGL(upper_bwd_kernel, dim3(cdiv(D, UW), cdiv(B, UR)), dim3(64 * UW), lds, stream, gates + i * 4 * bd, c + i * bd, c + (i + 1) * bd,
                       (const float*)dh[cur], dZ + i * bd, (const float*)dc[cur], w_hhT, dG + i * 4 * bd, dc[cur ^ 1], dh[cur ^ 1], B, D);
  RE2E_LAUNCH_CHECK();
  return RE2E_OK;
}
