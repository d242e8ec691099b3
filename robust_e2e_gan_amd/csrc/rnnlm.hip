// RNNLM shallow fusion at decode time (model/lm.py:125-146, e2e_decoder.py:270-285): the language model's step for the 1 .. 64 live
// hypotheses of a beam-search position.  Every product here has a handful of rows against megabytes of weights (two 650-unit LSTM
// cells and a 4233 x 650 output layer: 34 MB in fp32), so the weights are the streamed operand: a workgroup reads four weight rows
// straight into registers, once, in the widest loads their alignment allows, against up to 16 activation rows (L2-resident); the
// 4 x 16 lane-partial sums of a wave are reduced by a transposing butterfly (63 shuffles instead of 384) and the waves' totals meet
// in half a KB of LDS.  No workspace.
//   lm_cell_kernel     one workgroup per hidden unit j: gate rows j, j+H, j+2H, j+3H of W_ih and W_hh, then the cell -> h', c'
//   lm_out_kernel      one workgroup per four vocabulary rows: logits = W h + b
//   lm_lsm_kernel      row log-softmax (+ att + lm_weight * lm in the same pass)
//   lm_add_cands       local[k][j] += lm_weight * lm[k][cand[k][j]] (joint CTC/attention decoding)
#include "common.h"

namespace {

template <int VEC> struct VecT;
template <> struct VecT<4> { typedef float __attribute__((ext_vector_type(4))) type; };
template <> struct VecT<2> { typedef float __attribute__((ext_vector_type(2))) type; };
template <> struct VecT<1> { typedef float __attribute__((ext_vector_type(1))) type; };

#define LM_WAVES 2      // waves of a workgroup: they split the contraction of the workgroup's four weight rows between them (two: at 200+
                        // registers a SIMD holds two waves, and the 650 / 1059 workgroups of the recipe's widths are then resident at once)

// acc[g][r] += sum_k w[g][k] * a[r][k] over this lane's share of k: the workgroup's 128 lanes stride the row in VEC-wide pieces (a row
// of 650 is at most three pieces per lane, so few dependent load rounds stand between the launch and the reduction), the
// < VEC leftover columns go one per lane of the last wave.  Rows r >= nr alias row 0 (aoff), so that all R activation loads of a step
// issue without a branch.
template <int R, int VEC>
__device__ __forceinline__ void dot4(const float* const (&w)[4], int K, const float* __restrict__ act, const int (&aoff)[R], int wave, int lane,
                                     float (&acc)[4 * R]) {
  typedef typename VecT<VEC>::type vec_t;
  const int kv = K - K % VEC;
  for (int k = (wave * 64 + lane) * VEC; k < kv; k += LM_WAVES * 64 * VEC) {
    vec_t wv[4], av[R];
#pragma unroll
    for (int g = 0; g < 4; ++g) wv[g] = *reinterpret_cast<const vec_t*>(w[g] + k);
#pragma unroll
    for (int r = 0; r < R; ++r) av[r] = *reinterpret_cast<const vec_t*>(act + aoff[r] + k);
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
      for (int r = 0; r < R; ++r)
#pragma unroll
        for (int e = 0; e < VEC; ++e) acc[g * R + r] = fmaf(wv[g][e], av[r][e], acc[g * R + r]);
  }
  const int k = kv + lane;                                // K % VEC <= 3 leftover columns
  if (wave == LM_WAVES - 1 && k < K) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const float wv = w[g][k];
#pragma unroll
      for (int r = 0; r < R; ++r) acc[g * R + r] = fmaf(wv, act[aoff[r] + k], acc[g * R + r]);
    }
  }
}

// Sum v[i] over the 64 lanes for all NV (16 / 32 / 64) values at once: every step halves the values a lane still carries (the lane
// keeps the half its bit selects and hands the other half to its partner).  Returns the total of value i in the lanes
// i * (64 / NV) .. (i + 1) * (64 / NV) - 1.
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
  static_assert(NV == 16 || NV == 32 || NV == 64, "4 weight rows x 4 / 8 / 16 activation rows");
  reduce_step<NV, 32, NV>(v, lane);
  float s = v[0];
#pragma unroll
  for (int o = 64 / NV / 2; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  return s;
}

// The workgroup's total of every value: each wave reduces its own partial sums, wave 0 adds the LM_WAVES results in a fixed order.
// Valid in wave 0 only; `part` is reused by the next call (the leading barrier).
template <int NV>
__device__ __forceinline__ float reduce_block(float (&v)[NV], int wave, int lane, float (*part)[64]) {
  const float s = reduce_transposed<NV>(v, lane);
  __syncthreads();
  part[wave][lane] = s;
  __syncthreads();
  float t = 0.f;
  if (wave == 0) {
#pragma unroll
    for (int w = 0; w < LM_WAVES; ++w) t += part[w][lane];
  }
  return t;
}

// LSTMCell for n rows (torch gate order i, f, g, o).  x: dense rows (ids == nullptr) or an embedding table gathered by ids
// (an id outside [0, n_embed) gives a NaN row, never an out-of-bounds read).  h_prev / c_prev == nullptr: zeros.
// ZO (re2e_lm_lstm_cell_zo): x == nullptr is no input (b_ih alone contributes), and the new state is blended with the previous one,
// h = keep_h h' + (1 - keep_h) h_prev, c likewise (zoneout in evaluation mode, fsrnn.py:15-32).
template <int R, int VI, int VH, bool ZO>
__global__ __launch_bounds__(64 * LM_WAVES) void lm_cell_kernel(const float* __restrict__ x, long ldx, const int* __restrict__ ids, int n_embed, int I,
                                                      const float* __restrict__ w_ih, const float* __restrict__ w_hh,
                                                      const float* __restrict__ b_ih, const float* __restrict__ b_hh,
                                                      const float* __restrict__ h_prev, const float* __restrict__ c_prev, int n, int H,
                                                      float keep_h, float keep_c, float* __restrict__ h_out, float* __restrict__ c_out) {
  __shared__ float part[LM_WAVES][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int j = blockIdx.x;                               // one workgroup per hidden unit
  const float* wi[4];
  const float* wh[4];
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    wi[g] = w_ih + ((long)g * H + j) * I;
    wh[g] = w_hh + ((long)g * H + j) * H;
  }
  for (int row0 = 0; row0 < n; row0 += R) {
    const int nr = min(R, n - row0);
    int xoff[R], hoff[R];
    bool bad = false;                                     // of the row this lane finishes (lane r < nr)
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int rr = row0 + (r < nr ? r : 0);
      int src = rr;
      if (ids) {
        src = ids[rr];
        const bool oob = src < 0 || src >= n_embed;
        if (oob) src = 0;
        if (oob && lane == r) bad = true;
      }
      xoff[r] = src * (int)ldx;
      hoff[r] = rr * H;
    }
    // what the cell needs besides the products, asked for ahead of them (otherwise two more memory latencies behind the reduction)
    const bool fin = wave == 0 && lane < nr;
    const long o = (long)(row0 + (fin ? lane : 0)) * H + j;
    const float cp = (fin && c_prev) ? c_prev[o] : 0.f;
    const float hp = (ZO && fin && h_prev) ? h_prev[o] : 0.f;
    float bias[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) bias[g] = fin ? b_ih[g * H + j] + b_hh[g * H + j] : 0.f;
    float acc[4 * R];
#pragma unroll
    for (int i = 0; i < 4 * R; ++i) acc[i] = 0.f;
    if (!ZO || x) dot4<R, VI>(wi, I, x, xoff, wave, lane, acc);
    if (h_prev) dot4<R, VH>(wh, H, h_prev, hoff, wave, lane, acc);
    const float s = reduce_block<4 * R>(acc, wave, lane, part);
    constexpr int REP = 64 / (4 * R);                     // lanes that hold one (gate, row) total
    float gate[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) gate[g] = __shfl(s, ((g * R + (lane & (R - 1))) * REP) & 63, 64);
    if (fin) {
      const float gi = sigmoidf_(gate[0] + bias[0]);
      const float gf = sigmoidf_(gate[1] + bias[1]);
      const float gg = tanhf_(gate[2] + bias[2]);
      const float go = sigmoidf_(gate[3] + bias[3]);
      float c = gi * gg + gf * cp;
      float h = go * tanhf_(c);
      if (ZO) {
        h = h * keep_h + (1.f - keep_h) * hp;
        c = c * keep_c + (1.f - keep_c) * cp;
      }
      if (bad) c = h = __builtin_nanf("");
      c_out[o] = c;
      h_out[o] = h;
    }
  }
}

// logits[r][v] = w[v] . h[r] + b[v]: one workgroup per four vocabulary rows (the last one's rows beyond V alias row V - 1 and are not stored)
template <int R, int VEC>
__global__ __launch_bounds__(64 * LM_WAVES) void lm_out_kernel(const float* __restrict__ h, const float* __restrict__ w, const float* __restrict__ b, int n,
                                                     int V, int H, float* __restrict__ logits) {
  __shared__ float part[LM_WAVES][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int v0 = blockIdx.x * 4;
  const float* wr[4];
#pragma unroll
  for (int g = 0; g < 4; ++g) wr[g] = w + (long)min(v0 + g, V - 1) * H;
  constexpr int REP = 64 / (4 * R);
  for (int row0 = 0; row0 < n; row0 += R) {
    const int nr = min(R, n - row0);
    int hoff[R];
#pragma unroll
    for (int r = 0; r < R; ++r) hoff[r] = (row0 + (r < nr ? r : 0)) * H;
    float acc[4 * R];
#pragma unroll
    for (int i = 0; i < 4 * R; ++i) acc[i] = 0.f;
    dot4<R, VEC>(wr, H, h, hoff, wave, lane, acc);
    const float s = reduce_block<4 * R>(acc, wave, lane, part);
    const int idx = lane / REP, g = idx / R, r = idx % R;      // this lane's total: vocabulary row v0 + g, activation row row0 + r
    if (wave == 0 && lane % REP == 0 && r < nr && v0 + g < V) logits[(long)(row0 + r) * V + v0 + g] = s + b[v0 + g];
  }
}

// a + fl(w * x), the product and the sum rounded separately as the reference's two tensor operations are.  Contraction is switched off
// for the statement: __fadd_rn(a, __fmul_rn(w, x)) are a plain * and + to this compiler, which fuses them into one FMA by default.
__device__ __forceinline__ float add_scaled(float a, float w, float x) {
#pragma clang fp contract(off)
  const float p = w * x;
  return a + p;
}

// lsm[r][:] = log_softmax(logits[r][:]); comb[r][:] = att[r][:] + lm_weight * lsm[r][:] when asked (product and sum rounded
// separately, as the reference's two tensor operations are).  One workgroup per row; the first 8192 logits of a row stay in registers
// between the three passes.
#define LSM_THREADS 1024
#define LSM_KEEP 8
__global__ __launch_bounds__(LSM_THREADS) void lm_lsm_kernel(const float* __restrict__ logits, int V, const float* __restrict__ att,
                                                             float lm_weight, float* __restrict__ lsm, float* __restrict__ comb) {
  __shared__ float red[16];
  const long base = (long)blockIdx.x * V;
  const float* x = logits + base;
  float xv[LSM_KEEP];
  float m = -3.0e38f;
#pragma unroll
  for (int i = 0; i < LSM_KEEP; ++i) {
    const int v = threadIdx.x + i * LSM_THREADS;
    xv[i] = v < V ? x[v] : -3.0e38f;
    m = fmaxf(m, xv[i]);
  }
  for (int v = threadIdx.x + LSM_KEEP * LSM_THREADS; v < V; v += LSM_THREADS) m = fmaxf(m, x[v]);
  m = block_max(m, red);
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < LSM_KEEP; ++i)
    if (threadIdx.x + i * LSM_THREADS < V) s += expf(xv[i] - m);
  for (int v = threadIdx.x + LSM_KEEP * LSM_THREADS; v < V; v += LSM_THREADS) s += expf(x[v] - m);
  s = block_sum(s, red);
  const float l = m + logf(s);
#pragma unroll
  for (int i = 0; i < LSM_KEEP; ++i) {
    const int v = threadIdx.x + i * LSM_THREADS;
    if (v < V) {
      const float lp = xv[i] - l;
      lsm[base + v] = lp;
      if (comb) comb[base + v] = add_scaled(att[base + v], lm_weight, lp);
    }
  }
  for (int v = threadIdx.x + LSM_KEEP * LSM_THREADS; v < V; v += LSM_THREADS) {
    const float lp = x[v] - l;
    lsm[base + v] = lp;
    if (comb) comb[base + v] = add_scaled(att[base + v], lm_weight, lp);
  }
}

__global__ __launch_bounds__(256) void lm_add_cands_kernel(float* __restrict__ local, const float* __restrict__ lm, const int* __restrict__ cand,
                                                           int total, int ncand, int V, float lm_weight) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int c = cand[i];
  if (c < 0 || c >= V) { local[i] = __builtin_nanf(""); return; }
  local[i] = add_scaled(local[i], lm_weight, lm[(long)(i / ncand) * V + c]);
}

inline bool aligned(const void* p, int bytes) { return p == nullptr || ((uintptr_t)p % bytes) == 0; }
// widest load (floats) every row of a (rows x K, leading dimension ld) operand starts aligned for
inline int vec_width(const void* p, long ld) {
  if (ld % 4 == 0 && aligned(p, 16)) return 4;
  if (ld % 2 == 0 && aligned(p, 8)) return 2;
  return 1;
}

// The form a call runs in, chosen on the host from the row count and from what every row of every operand is aligned for: the one
// place lm_cell_entry, re2e_lm_output and re2e_lm_plan take it from.
inline int rows_per_trip(int n) { return n <= 4 ? 4 : n <= 8 ? 8 : 16; }      // R: activation rows a workgroup carries per trip of its row0 loop
struct CellForm { int R, vi, vh, grid; };                                       // lm_cell_kernel<R, vi, vh, .>, one workgroup per hidden unit
struct OutForm { int R, vec, grid; };                                           // lm_out_kernel<R, vec>, one workgroup per four vocabulary rows
// (vi, vh) is one of the four instantiated pairs (4,4), (4,2), (2,2), (1,1): the widest that both operands of each product allow
inline CellForm cell_form(const float* x, long ldx, int I, const float* w_ih, const float* w_hh, const float* h_prev, int n, int H) {
  const int vi = x ? min(vec_width(w_ih, I), vec_width(x, ldx)) : 1;
  const int vh = min(vec_width(w_hh, H), vec_width(h_prev, H));
  CellForm f = {rows_per_trip(n), 1, 1, H};
  if (vi == 4 && vh == 4) { f.vi = 4; f.vh = 4; }
  else if (vi == 4 && vh == 2) { f.vi = 4; f.vh = 2; }
  else if (vi >= 2 && vh >= 2) { f.vi = 2; f.vh = 2; }
  return f;
}
inline OutForm out_form(const float* h, const float* w, int n, int V, int H) {
  return OutForm{rows_per_trip(n), min(vec_width(w, H), vec_width(h, H)), cdiv(V, 4)};
}

template <int R, bool ZO>
void launch_cell(const CellForm& f, hipStream_t st, const float* x, long ldx, const int* ids, int n_embed, int I, const float* w_ih,
                 const float* w_hh, const float* b_ih, const float* b_hh, const float* h_prev, const float* c_prev, int n, int H, float keep_h,
                 float keep_c, float* h_out, float* c_out) {
#define RE2E_LM_CELL(VI, VH)                                                                                                             \
  hipLaunchKernelGGL((lm_cell_kernel<R, VI, VH, ZO>), dim3(f.grid), dim3(64 * LM_WAVES), 0, st, x, ldx, ids, n_embed, I, w_ih, w_hh, b_ih, b_hh, h_prev, \
                     c_prev, n, H, keep_h, keep_c, h_out, c_out)
  if (f.vi == 4 && f.vh == 4) RE2E_LM_CELL(4, 4);
  else if (f.vi == 4 && f.vh == 2) RE2E_LM_CELL(4, 2);
  else if (f.vi == 2 && f.vh == 2) RE2E_LM_CELL(2, 2);
  else RE2E_LM_CELL(1, 1);
#undef RE2E_LM_CELL
}

template <int R>
void launch_out(const OutForm& f, hipStream_t st, const float* h, const float* w, const float* b, int n, int V, int H, float* logits) {
  const dim3 grid(f.grid);
  if (f.vec == 4) hipLaunchKernelGGL((lm_out_kernel<R, 4>), grid, dim3(64 * LM_WAVES), 0, st, h, w, b, n, V, H, logits);
  else if (f.vec == 2) hipLaunchKernelGGL((lm_out_kernel<R, 2>), grid, dim3(64 * LM_WAVES), 0, st, h, w, b, n, V, H, logits);
  else hipLaunchKernelGGL((lm_out_kernel<R, 1>), grid, dim3(64 * LM_WAVES), 0, st, h, w, b, n, V, H, logits);
}

template <bool ZO>
int lm_cell_entry(const float* x, long ldx, const int* ids_dev, int n_embed, int I, const float* w_ih, const float* w_hh, const float* b_ih,
                  const float* b_hh, const float* h_prev, const float* c_prev, int n, int H, float keep_h, float keep_c, float* h_out, float* c_out,
                  hipStream_t stream) {
  RE2E_CHECK_ARG((x || ZO) && (w_ih || !x) && w_hh && b_ih && b_hh && h_out && c_out, "null operand");
  RE2E_CHECK_ARG(x || !ids_dev, "ids without a table");
  if (!x) { I = 1; ldx = 1; }
  RE2E_CHECK_ARG(n > 0 && n <= 64 && I > 0 && H > 0 && ldx >= I, "bad shape (1 <= n <= 64)");
  RE2E_CHECK_ARG(!ids_dev || n_embed > 0, "embedding gather needs the table's row count");
  RE2E_CHECK_ARG((long)(ids_dev ? n_embed : n) * ldx < (1L << 31) && (long)n * H < (1L << 31), "operand beyond 32-bit element offsets");
  RE2E_CHECK_ARG(h_out != h_prev && c_out != h_prev, "h_prev is read by every workgroup: the outputs must not alias it");
  const CellForm f = cell_form(x, ldx, I, w_ih, w_hh, h_prev, n, H);
#define RE2E_LM_ARGS f, stream, x, ldx, ids_dev, n_embed, I, w_ih, w_hh, b_ih, b_hh, h_prev, c_prev, n, H, keep_h, keep_c, h_out, c_out
  if (f.R == 4) launch_cell<4, ZO>(RE2E_LM_ARGS);
  else if (f.R == 8) launch_cell<8, ZO>(RE2E_LM_ARGS);
  else launch_cell<16, ZO>(RE2E_LM_ARGS);
#undef RE2E_LM_ARGS
  RE2E_LAUNCH_CHECK();
  return RE2E_OK;
}

}  // namespace

extern "C" int re2e_lm_lstm_cell(const float* x, long ldx, const int* ids_dev, int n_embed, int I, const float* w_ih, const float* w_hh,
                                 const float* b_ih, const float* b_hh, const float* h_prev, const float* c_prev, int n, int H, float* h_out,
                                 float* c_out, hipStream_t stream) {
  return lm_cell_entry<false>(x, ldx, ids_dev, n_embed, I, w_ih, w_hh, b_ih, b_hh, h_prev, c_prev, n, H, 1.f, 1.f, h_out, c_out, stream);
}

extern "C" int re2e_lm_lstm_cell_zo(const float* x, long ldx, const int* ids_dev, int n_embed, int I, const float* w_ih, const float* w_hh,
                                    const float* b_ih, const float* b_hh, const float* h_prev, const float* c_prev, int n, int H, float keep_h,
                                    float keep_c, float* h_out, float* c_out, hipStream_t stream) {
  return lm_cell_entry<true>(x, ldx, ids_dev, n_embed, I, w_ih, w_hh, b_ih, b_hh, h_prev, c_prev, n, H, keep_h, keep_c, h_out, c_out, stream);
}

extern "C" int re2e_lm_output(const float* h, const float* w, const float* b, int n, int V, int H, float* logits, hipStream_t stream) {
  RE2E_CHECK_ARG(h && w && b && logits, "null operand");
  RE2E_CHECK_ARG(n > 0 && n <= 64 && V > 0 && H > 0, "bad shape (1 <= n <= 64)");
  const OutForm f = out_form(h, w, n, V, H);
  if (f.R == 4) launch_out<4>(f, stream, h, w, b, n, V, H, logits);
  else if (f.R == 8) launch_out<8>(f, stream, h, w, b, n, V, H, logits);
  else launch_out<16>(f, stream, h, w, b, n, V, H, logits);
  RE2E_LAUNCH_CHECK();
  return RE2E_OK;
}

extern "C" int re2e_lm_plan(int kind, const float* x, long ldx, int I, const float* w_ih, const float* w_hh, const float* h_prev, int n, int H, int V,
                            char* out, size_t out_bytes) {
  RE2E_CHECK_ARG(out && out_bytes > 0, "no output buffer");
  RE2E_CHECK_ARG(kind == RE2E_LM_PLAN_CELL || kind == RE2E_LM_PLAN_CELL_ZO || kind == RE2E_LM_PLAN_OUTPUT, "unknown kind");
  RE2E_CHECK_ARG(n > 0 && n <= 64 && H > 0, "bad shape (1 <= n <= 64)");
  int len;
  if (kind == RE2E_LM_PLAN_OUTPUT) {
    RE2E_CHECK_ARG(h_prev && w_hh && V > 0, "the output layer needs h, w and V > 0");
    const OutForm f = out_form(h_prev, w_hh, n, V, H);
    len = snprintf(out, out_bytes, "family=lm_out rows=%d vec=%d grid=%dx1x1 block=%d trips=%d", f.R, f.vec, f.grid, 64 * LM_WAVES, cdiv(n, f.R));
  } else {
    const bool zo = kind == RE2E_LM_PLAN_CELL_ZO;
    RE2E_CHECK_ARG((x || zo) && (w_ih || !x) && w_hh, "null operand");
    if (!x) { I = 1; ldx = 1; }
    RE2E_CHECK_ARG(I > 0 && ldx >= I, "bad shape (ldx >= I > 0)");
    const CellForm f = cell_form(x, ldx, I, w_ih, w_hh, h_prev, n, H);
    len = snprintf(out, out_bytes, "family=lm_cell zo=%d rows=%d vi=%d vh=%d grid=%dx1x1 block=%d trips=%d", zo ? 1 : 0, f.R, f.vi, f.vh, f.grid,
                   64 * LM_WAVES, cdiv(n, f.R));
  }
  RE2E_CHECK_ARG(len > 0 && (size_t)len < out_bytes, "output buffer too small");
  return RE2E_OK;
}

extern "C" int re2e_lm_log_softmax_combine(const float* logits, int n, int V, const float* att, float lm_weight, float* lsm, float* comb,
                                           hipStream_t stream) {
  RE2E_CHECK_ARG(logits && lsm && n > 0 && V > 0, "bad args");
  RE2E_CHECK_ARG((att != nullptr) == (comb != nullptr), "att and comb go together");
  hipLaunchKernelGGL(lm_lsm_kernel, dim3(n), dim3(LSM_THREADS), 0, stream, logits, V, att, lm_weight, lsm, comb);
  RE2E_LAUNCH_CHECK();
  return RE2E_OK;
}

extern "C" int re2e_lm_add_cands(float* local, const float* lm, const int* cand_dev, int n, int ncand, int V, float lm_weight,
                                 hipStream_t stream) {
  RE2E_CHECK_ARG(local && lm && cand_dev && n > 0 && ncand > 0 && V > 0, "bad args");
  RE2E_CHECK_ARG((long)n * ncand < (1L << 30), "too many candidates");
  const int total = n * ncand;
  hipLaunchKernelGGL(lm_add_cands_kernel, dim3(cdiv(total, 256)), dim3(256), 0, stream, local, lm, cand_dev, total, ncand, V, lm_weight);
  RE2E_LAUNCH_CHECK();
  return RE2E_OK;
}
