// Word-level language models in the beam search (model/extlm.py here; extlm.py:75-216 upstream): LookAheadWordLM and MultiLevelLM for the
// 1 .. 64 live hypotheses of a position.  The lexical tree is flat int32 arrays (node 0 = root; per node the word id or -1, the word-set
// range (lo, hi] as indices into the cumulative word probabilities -- lo < 0 marks the root, "sum_prob = 1" -- and a CSR child list with
// ascending labels); a hypothesis holds a node id, -1 = no path in the tree (open-vocabulary mode).  No workspace; every tree or
// vocabulary index that reaches a kernel is checked against its array before it is used (a bad one gives NaN, never a stray read).
//   wlm_transition_kernel    (node, label) -> new node, the word id the word LM is fed at a <space>, the at-space flag: one thread per row
//   wlm_cumsum_kernel        inclusive prefix sums of softmax(word logits), one workgroup per row, running sums in fp64
//   wlm_lookahead_kernel     extlm.py:195-216: the label log-probabilities of a node from the cumulative word probabilities
//   wlm_multilevel_kernel    extlm.py:133-143: subwordlm_weight * log-softmax with the <space> / <eos> columns from the word LM
#include "common.h"

namespace {

#define WLM_BAD (-1)        // at_space value of a row whose label or node was out of range: NaN downstream

__global__ __launch_bounds__(64) void wlm_transition_kernel(const int* __restrict__ node_prev, const int* __restrict__ labels, int n, int Vc, int space,
                                                            int word_unk, const int* __restrict__ wid, const int* __restrict__ child_off,
                                                            const int* __restrict__ child_label, const int* __restrict__ child_node, int N, int nchild,
                                                            int* __restrict__ node_new, int* __restrict__ word_in, int* __restrict__ at_space) {
  const int r = blockIdx.x * 64 + threadIdx.x;
  if (r >= n) return;
  const int x = labels[r];
  const int nd = node_prev ? node_prev[r] : 0;            // no previous state: every row stands at the root
  int nn = -1, w = word_unk, sp = 0;
  if (x < 0 || x >= Vc || nd < -1 || nd >= N) {
    sp = WLM_BAD;
  } else if (x == space) {                                // inter-word transition: back to the root, the finished word (or <unk>) goes to the word LM
    sp = 1;
    nn = 0;
    if (nd >= 0 && wid[nd] >= 0) w = wid[nd];
  } else if (nd >= 0) {                                   // intra-word transition: the child with this label, or no path
    int lo = child_off[nd], hi = child_off[nd + 1];
    if (lo < 0 || hi > nchild || lo > hi) {
      sp = WLM_BAD;
    } else {
      while (lo < hi) {                                   // labels ascend inside a node
        const int mid = (lo + hi) >> 1;
        const int l = child_label[mid];
        if (l == x) { nn = child_node[mid]; break; }
        if (l < x) lo = mid + 1; else hi = mid;
      }
      if (nn < -1 || nn >= N) { nn = -1; sp = WLM_BAD; }
    }
  }
  node_new[r] = nn;
  word_in[r] = w;
  at_space[r] = sp;
}

// Inclusive scan of one double per lane over the wave.
__device__ __forceinline__ double wave_scan_f64(double v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const double u = __shfl_up(v, o, 64);
    if (lane >= o) v += u;
  }
  return v;
}

#define CS_THREADS 1024
#define CS_WAVES (CS_THREADS / 64)
#define CS_CHUNK 4          // consecutive elements per thread and pass: a pass of the workgroup covers 4096 elements

// cumsum[dst_rows[j]][v] = sum_{u <= v} softmax(logits[j])[u].  The probabilities are fp32 (expf(x - max) / sum, the sum accumulated in fp64 and
// rounded once); every running sum -- a thread's chunk, the wave scan, the carry between waves and between passes -- is fp64 and is rounded to
// fp32 only at the store.  A probability enters the scan cut to a multiple of 2^-52 (it loses less than 2^-52: 1.4e-11 over a row of 65 k):
// every partial sum is then a multiple of 2^-52 below 2, which fp64 holds exactly, so the additions do not round, the result does not depend
// on how the row is cut into threads, waves and passes, `incl - t` below is exact, and a row can never decrease (a rounded fp64 scan can, by
// one fp32 step where a tiny probability follows a large one: a negative word mass).
__global__ __launch_bounds__(CS_THREADS) void wlm_cumsum_kernel(const float* __restrict__ logits, int Vw, const int* __restrict__ dst_rows, int n,
                                                                float* __restrict__ cumsum) {
  __shared__ float red[16];
  __shared__ double dred[CS_WAVES];
  const int j = blockIdx.x;
  const int dst = dst_rows ? dst_rows[j] : j;
  if (dst < 0 || dst >= n) return;                        // (uniform over the workgroup) never a store outside the buffer
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* x = logits + (long)j * Vw;
  float* out = cumsum + (long)dst * Vw;
  float m = -3.0e38f;
  for (int v = tid; v < Vw; v += CS_THREADS) m = fmaxf(m, x[v]);
  m = block_max(m, red);
  double s = 0.0;
  for (int v = tid; v < Vw; v += CS_THREADS) s += (double)expf(x[v] - m);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if (lane == 0) dred[wave] = s;
  __syncthreads();
  double tot = 0.0;
#pragma unroll
  for (int w = 0; w < CS_WAVES; ++w) tot += dred[w];
  const float sum = (float)tot;
  __syncthreads();                                        // dred is reused below
  double carry = 0.0;
  for (int base = 0; base < Vw; base += CS_THREADS * CS_CHUNK) {
    const int v0 = base + tid * CS_CHUNK;
    double p[CS_CHUNK];
    double t = 0.0;
#pragma unroll
    for (int e = 0; e < CS_CHUNK; ++e) {
      const float pe = v0 + e < Vw ? expf(x[v0 + e] - m) / sum : 0.f;
      t += trunc((double)pe * 0x1p52) * 0x1p-52;
      p[e] = t;                                           // the thread's own inclusive prefix
    }
    const double incl = wave_scan_f64(t, lane);
    if (lane == 63) dred[wave] = incl;
    __syncthreads();
    double before = carry;                                // everything in front of this thread's chunk
    double pass = 0.0;
#pragma unroll
    for (int w = 0; w < CS_WAVES; ++w) {
      if (w < wave) before += dred[w];
      pass += dred[w];
    }
    before += incl - t;
#pragma unroll
    for (int e = 0; e < CS_CHUNK; ++e)
      if (v0 + e < Vw) out[v0 + e] = (float)(before + p[e]);
    carry += pass;
    __syncthreads();
  }
}

// c[hi] - c[lo] in one fp32 subtraction; an index outside the row gives NaN
__device__ __forceinline__ float cdiff(const float* __restrict__ c, int hi, int lo, int Vw) {
  if (hi < 0 || hi >= Vw || lo < 0 || lo >= Vw) return __builtin_nanf("");
  return __fsub_rn(c[hi], c[lo]);
}

#define LA_THREADS 256
#define WLM_LOGZERO (-10000000000.0f)
#define WLM_ZERO (1.0e-10f)

__global__ __launch_bounds__(LA_THREADS) void wlm_lookahead_kernel(const float* __restrict__ cumsum, int Vw, const int* __restrict__ node,
                                                                   const int* __restrict__ at_space, const int* __restrict__ wid,
                                                                   const int* __restrict__ lo, const int* __restrict__ hi,
                                                                   const int* __restrict__ child_off, const int* __restrict__ child_label,
                                                                   const int* __restrict__ child_node, int N, int nchild, int Vc, int space, int eos,
                                                                   int word_unk, int word_eos, float oov_penalty, int open_vocab,
                                                                   float* __restrict__ log_y) {
  const int r = blockIdx.x;
  float* y = log_y + (long)r * Vc;
  const int nd = node[r], sp = at_space[r];
  int c0 = 0, c1 = 0;
  bool bad = sp == WLM_BAD || nd < -1 || nd >= N;
  if (!bad && nd >= 0) {
    c0 = child_off[nd];
    c1 = child_off[nd + 1];
    bad = c0 < 0 || c1 > nchild || c0 > c1;
  }
  if (bad || nd < 0) {                                    // uniform over the workgroup
    const float v = bad ? __builtin_nanf("") : (open_vocab ? 0.f : WLM_LOGZERO);   // no path in the tree: probability one, or none
    for (int k = threadIdx.x; k < Vc; k += LA_THREADS) y[k] = v;
    return;
  }
  const float* c = cumsum + (long)r * Vw;
  const float sum_prob = lo[nd] < 0 ? 1.0f : cdiff(c, hi[nd], lo[nd], Vw);                  // the root: all words
  const float unk = __fmul_rn(cdiff(c, word_unk, word_unk - 1, Vw), oov_penalty);           // the default of every label
  const int w = wid[nd];
  float y_space = 0.f, y_eos = 0.f;
  const bool fix = w >= 0 || sp == 1;
  if (w >= 0) {                                           // word end: the word's own probability for <space>, times P(<eos>) for <eos>
    y_space = __fdiv_rn(cdiff(c, w, w - 1, Vw), sum_prob);
    y_eos = __fmul_rn(y_space, cdiff(c, word_eos, word_eos - 1, Vw));
  } else if (sp == 1) {
    y_space = y_eos = WLM_ZERO;
  }
  for (int k = threadIdx.x; k < Vc; k += LA_THREADS) {
    float v = unk;
    int a = c0, b = c1;
    while (a < b) {                                       // is label k a child of the node?
      const int mid = (a + b) >> 1;
      const int l = child_label[mid];
      if (l == k) {
        const int ch = child_node[mid];
        v = (ch < 0 || ch >= N) ? __builtin_nanf("") : __fdiv_rn(cdiff(c, hi[ch], lo[ch], Vw), sum_prob);
        break;
      }
      if (l < k) a = mid + 1; else b = mid;
    }
    if (fix && k == space) v = y_space;
    if (fix && k == eos) v = y_eos;                       // (written after <space>, as upstream)
    y[k] = logf(v);
  }
}

// log_y[r][:] = weight * lsm[r][:] with the <space> / <eos> columns from the word LM's log-probabilities; clm_out[r] = the character LM's
// log-probability of the word so far (0 right after a <space>).
__global__ __launch_bounds__(LA_THREADS) void wlm_multilevel_kernel(const float* __restrict__ lsm, const float* __restrict__ wlm, int Vw,
                                                                    const int* __restrict__ node, const int* __restrict__ at_space,
                                                                    const int* __restrict__ wid, int N, const float* __restrict__ clm_prev,
                                                                    const float* __restrict__ log_y_prev, const int* __restrict__ labels, int Vc,
                                                                    int space, int eos, int word_unk, int word_eos, float weight, float log_oov,
                                                                    int open_vocab, float* __restrict__ log_y, float* __restrict__ clm_out) {
  const int r = blockIdx.x;
  float* y = log_y + (long)r * Vc;
  const int nd = node[r], sp = at_space[r];
  const int x = labels ? labels[r] : space;
  const bool bad = sp == WLM_BAD || nd < -1 || nd >= N || x < 0 || x >= Vc || word_unk < 0 || word_unk >= Vw || word_eos < 0 || word_eos >= Vw;
  const bool dead = !bad && sp == 0 && nd < 0 && !open_vocab;          // no path and no open vocabulary: zero probabilities
  if (bad || dead) {
    const float v = bad ? __builtin_nanf("") : WLM_LOGZERO;
    for (int k = threadIdx.x; k < Vc; k += LA_THREADS) y[k] = v;
    if (threadIdx.x == 0) clm_out[r] = bad ? v : 0.f;
    return;
  }
  float clm = 0.f;
  if (sp == 0 && clm_prev) clm = __fadd_rn(clm_prev[r], log_y_prev[(long)r * Vc + x]);
  float y_space = WLM_LOGZERO, y_eos = WLM_LOGZERO;
  if (sp == 0) {
    const float* wl = wlm + (long)r * Vw;
    const int w = nd >= 0 ? wid[nd] : -1;
    if (w >= Vw) y_space = __builtin_nanf("");
    else if (w >= 0) y_space = __fsub_rn(wl[w], clm);
    else y_space = __fadd_rn(wl[word_unk], log_oov);
    y_eos = __fadd_rn(y_space, wl[word_eos]);
  }
  const float* in = lsm + (long)r * Vc;
  for (int k = threadIdx.x; k < Vc; k += LA_THREADS) {
    float v = __fmul_rn(in[k], weight);
    if (k == space) v = y_space;
    if (k == eos) v = y_eos;
    y[k] = v;
  }
  if (threadIdx.x == 0) clm_out[r] = clm;
}

}  // namespace

extern "C" int re2e_wlm_transition(const int* node_prev, const int* labels, int n, int Vc, int space, int word_unk, const int* wid,
                                   const int* child_off, const int* child_label, const int* child_node, int N, int nchild, int* node_new,
                                   int* word_in, int* at_space, hipStream_t stream) {
  RE2E_CHECK_ARG(labels && wid && child_off && child_label && child_node && node_new && word_in && at_space, "null operand");
  RE2E_CHECK_ARG(n > 0 && Vc > 0 && N > 0 && nchild >= 0, "bad shape");
  hipLaunchKernelGGL(wlm_transition_kernel, dim3(cdiv(n, 64)), dim3(64), 0, stream, node_prev, labels, n, Vc, space, word_unk, wid, child_off,
                     child_label, child_node, N, nchild, node_new, word_in, at_space);
  RE2E_LAUNCH_CHECK();
  return RE2E_OK;
}

extern "C" int re2e_wlm_softmax_cumsum(const float* logits, int m, int Vw, const int* dst_rows, int n, float* cumsum, hipStream_t stream) {
  RE2E_CHECK_ARG(logits && cumsum, "null operand");
  RE2E_CHECK_ARG(m > 0 && n > 0 && Vw > 0 && (dst_rows || m <= n), "bad shape (without dst_rows the m rows go to rows 0 .. m-1 of n)");
  hipLaunchKernelGGL(wlm_cumsum_kernel, dim3(m), dim3(CS_THREADS), 0, stream, logits, Vw, dst_rows, n, cumsum);
  RE2E_LAUNCH_CHECK();
  return RE2E_OK;
}

extern "C" int re2e_wlm_lookahead(const float* cumsum, int n, int Vw, const int* node, const int* at_space, const int* wid, const int* lo,
                                  const int* hi, const int* child_off, const int* child_label, const int* child_node, int N, int nchild, int Vc,
                                  int space, int eos, int word_unk, int word_eos, float oov_penalty, int open_vocab, float* log_y,
                                  hipStream_t stream) {
  RE2E_CHECK_ARG(cumsum && node && at_space && wid && lo && hi && child_off && child_label && child_node && log_y, "null operand");
  RE2E_CHECK_ARG(n > 0 && Vw > 0 && Vc > 0 && N > 0 && nchild >= 0, "bad shape");
  hipLaunchKernelGGL(wlm_lookahead_kernel, dim3(n), dim3(LA_THREADS), 0, stream, cumsum, Vw, node, at_space, wid, lo, hi, child_off, child_label,
                     child_node, N, nchild, Vc, space, eos, word_unk, word_eos, oov_penalty, open_vocab, log_y);
  RE2E_LAUNCH_CHECK();
  return RE2E_OK;
}

extern "C" int re2e_wlm_multilevel_fix(const float* lsm, const float* wlm_logprobs, int n, int Vw, const int* node, const int* at_space,
                                       const int* wid, int N, const float* clm_prev, const float* log_y_prev, const int* labels, int Vc,
                                       int space, int eos, int word_unk, int word_eos, float subwordlm_weight, float log_oov_penalty,
                                       int open_vocab, float* log_y, float* clm_out, hipStream_t stream) {
  RE2E_CHECK_ARG(lsm && wlm_logprobs && node && at_space && wid && log_y && clm_out, "null operand");
  RE2E_CHECK_ARG(n > 0 && Vw > 0 && Vc > 0 && N > 0, "bad shape");
  RE2E_CHECK_ARG((clm_prev != nullptr) == (log_y_prev != nullptr) && (clm_prev == nullptr || labels != nullptr),
                 "clm_prev, log_y_prev and labels go together (all NULL: the initial position)");
  RE2E_CHECK_ARG(log_y != lsm && log_y != log_y_prev, "log_y must not alias its inputs");
  hipLaunchKernelGGL(wlm_multilevel_kernel, dim3(n), dim3(LA_THREADS), 0, stream, lsm, wlm_logprobs, Vw, node, at_space, wid, N, clm_prev, log_y_prev,
                     labels, Vc, space, eos, word_unk, word_eos, subwordlm_weight, log_oov_penalty, open_vocab, log_y, clm_out);
  RE2E_LAUNCH_CHECK();
  return RE2E_OK;
}
