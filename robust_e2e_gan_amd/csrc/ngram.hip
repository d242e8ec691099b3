// N-gram (ARPA back-off) language models in the beam search (model/ngram.py here; NgramCharacterKenLM, extlm.py:46-72 upstream, which asks kenlm
// for one label of one hypothesis at a time on the host).  The whole model is flat arrays in HBM, in the style of the lexical tree of wordlm.hip:
// node 0 is the root (the empty context), every n-gram of length 1 .. order-1 is a node; per node its back-off weight bo, the node of its
// longest proper suffix that is a node (bo_node) and a CSR list of successors with ascending labels, each with its log-probability and the node
// of the longest suffix of context.label that is a node (succ_next).  The root's successors are the dense rows uni_logp / uni_next.  A hypothesis
// holds a node id.  No workspace; every index that is read from the tables is checked against its array before it is used (a bad one gives the row
// NaN scores and state -1, never a stray read), and a back-off chain is followed for at most NG_MAXLEV nodes (a cycle in a damaged bo_node ends as
// a bad row, not as a hang).
//   ngram_step_kernel        one search position: advance n rows by their labels, then the V log-probabilities after each row (+ att + w * lp)
//   ngram_score_seqs_kernel  summed log-probability of S whole label sequences, one thread per sequence, fp32 terms added in double
#include "common.h"

namespace {

#define NG_MAXLEV 8          // orders 1 .. 8: a back-off chain has at most 7 nodes below the root, plus the root
#define NG_THREADS 256
#define NG_TILE 4096         // labels per workgroup: the tile of the row it assembles in LDS (16 KB)

struct NgTables {
  const float* uni_logp; const int* uni_next; const float* bo; const int* bo_node; const int* succ_off; const int* succ_label;
  const float* succ_logp; const int* succ_next; int N, nsucc, V;
};

// The successor range of node `nd` (in [0, N)), checked: false when the offsets do not describe a range inside the arrays.
__device__ __forceinline__ bool ng_range(const NgTables& t, int nd, int& a, int& b) {
  a = t.succ_off[nd];
  b = t.succ_off[nd + 1];
  return a >= 0 && b <= t.nsucc && a <= b;
}

// First entry of [a, b) whose label is >= x (labels ascend inside a node).
__device__ __forceinline__ int ng_lower_bound(const int* __restrict__ lab, int a, int b, int x) {
  while (a < b) {
    const int mid = (a + b) >> 1;
    if (lab[mid] < x) a = mid + 1; else b = mid;
  }
  return a;
}

// The node `lev` back-off steps above `s` (s in [0, N)): -1 when the chain leaves [0, N) on the way, the root stays the root.
__device__ __forceinline__ int ng_ancestor(const NgTables& t, int s, int lev) {
  int nd = s;
  for (int i = 0; i < lev && nd > 0; ++i) {
    nd = t.bo_node[nd];
    if (nd < 0 || nd >= t.N) return -1;
  }
  return nd;
}

// p(x | node) by Katz back-off from node s (in [0, N)), x in [0, V): the back-offs of the nodes that do not hold x are added in fp32 from the deep
// end, then the log-probability (one more fp32 addition; at s itself 0 + logp).  next: the node after x; false: a table index was out of range.
__device__ __forceinline__ bool ng_walk(const NgTables& t, int s, int x, float& term, int& next) {
  float acc = 0.f;
  int nd = s;
  for (int lev = 0; lev < NG_MAXLEV; ++lev) {
    if (nd == 0) {
      term = __fadd_rn(acc, t.uni_logp[x]);
      next = t.uni_next[x];
      return next >= 0 && next < t.N;
    }
    int a, b;
    if (!ng_range(t, nd, a, b)) return false;
    const int e = ng_lower_bound(t.succ_label, a, b, x);
    if (e < b && t.succ_label[e] == x) {
      term = __fadd_rn(acc, t.succ_logp[e]);
      next = t.succ_next[e];
      return next >= 0 && next < t.N;
    }
    acc = __fadd_rn(acc, t.bo[nd]);
    nd = t.bo_node[nd];
    if (nd < 0 || nd >= t.N) return false;
  }
  return false;                 // no root within NG_MAXLEV nodes
}

// a + fl(w * x), the product and the sum rounded separately (e2e_decoder.py:272 is two tensor operations).  Contraction is switched off for the
// statement: __fadd_rn(a, __fmul_rn(w, x)) are a plain * and + to this compiler, which fuses them into one FMA by default (as in rnnlm.hip).
__device__ __forceinline__ float add_scaled(float a, float w, float x) {
#pragma clang fp contract(off)
  const float p = w * x;
  return a + p;
}

// Workgroup (r, tile): advances row r (every workgroup of the row repeats the few loads of that) and assembles labels [t0, t0 + len) of its
// scores in LDS: the root's dense row first, then the chain's levels shallow to deep, a deeper level overwriting a shallower one (the deepest
// context that holds a label wins); one coalesced pass writes the tile out.
__global__ __launch_bounds__(NG_THREADS) void ngram_step_kernel(NgTables t, const int* __restrict__ state_in, const int* __restrict__ x, int tiles,
                                                                const float* __restrict__ att, float lm_weight, int* __restrict__ state_out,
                                                                float* __restrict__ lp_out, float* __restrict__ comb_out) {
  __shared__ float tile[NG_TILE];
  __shared__ int sh_next[NG_MAXLEV];          // transition: the successor's node found at level l of the old chain, -1 none, -2 bad table
  __shared__ int sh_node[NG_MAXLEV];          // the new chain d0, d1, .. root
  __shared__ float sh_pre[NG_MAXLEV];         // bo[d0] + .. + bo[d_{j-1}]: what level j adds to its log-probabilities
  __shared__ int sh_a[NG_MAXLEV], sh_b[NG_MAXLEV];      // level j's successor entries whose labels fall into this tile
  __shared__ int sh_levels;                   // nodes of the new chain, the root included; 0: a bad row
  __shared__ int sh_bad;                      // a level's offsets do not describe a range: a bad row as well
  const int tid = threadIdx.x;
  const int r = blockIdx.x / tiles, tl = blockIdx.x - r * tiles;
  const int t0 = tl * NG_TILE, len = min(NG_TILE, t.V - t0);
  const int s = state_in ? state_in[r] : 0;
  const int xr = x[r];
  const bool ok_in = s >= 0 && s < t.N && xr >= 0 && xr < t.V;

  // ---- the transition: level l of the old chain looks for the label on lane l
  if (tid < NG_MAXLEV) {
    int found = -1;
    if (ok_in) {
      const int nd = ng_ancestor(t, s, tid);
      if (nd < 0) {
        found = -2;
      } else if (nd == 0) {
        found = t.uni_next[xr];
        if (found < 0 || found >= t.N) found = -2;
      } else {
        int a, b;
        if (!ng_range(t, nd, a, b)) {
          found = -2;
        } else {
          const int e = ng_lower_bound(t.succ_label, a, b, xr);
          if (e < b && t.succ_label[e] == xr) {
            found = t.succ_next[e];
            if (found < 0 || found >= t.N) found = -2;
          }
        }
      }
    }
    sh_next[tid] = found;
  }
  __syncthreads();
  // ---- the new chain and its running back-off sums (a handful of dependent loads: one thread)
  if (tid == 0) {
    int d = -1;
    for (int l = 0; l < NG_MAXLEV && ok_in; ++l) {
      if (sh_next[l] == -1) continue;           // (the root's level always answers, so a good row ends here before NG_MAXLEV)
      d = sh_next[l];
      break;
    }
    int levels = 0;
    if (d >= 0) {
      float acc = 0.f;
      int nd = d;
      for (int l = 0; l < NG_MAXLEV; ++l) {
        sh_node[l] = nd;
        sh_pre[l] = acc;
        if (nd == 0) { levels = l + 1; break; }
        acc = __fadd_rn(acc, t.bo[nd]);
        nd = t.bo_node[nd];
        if (nd < 0 || nd >= t.N) break;
      }
    }
    sh_levels = levels;
    sh_bad = 0;
  }
  __syncthreads();
  const int levels = sh_levels;
  // ---- the part of each level's successor list that falls into this tile
  if (tid < levels - 1) {
    int a, b;
    if (ng_range(t, sh_node[tid], a, b)) {
      sh_a[tid] = ng_lower_bound(t.succ_label, a, b, t0);
      sh_b[tid] = ng_lower_bound(t.succ_label, a, b, t0 + len);
    } else {
      sh_a[tid] = sh_b[tid] = 0;
      sh_bad = 1;                               // (read after the next barrier)
    }
  }
  __syncthreads();
  const bool good = levels > 0 && !sh_bad;
  if (tid == 0 && tl == 0) state_out[r] = good ? sh_node[0] : -1;
  if (good) {
    const float pre_root = sh_pre[levels - 1];
    for (int k = tid; k < len; k += NG_THREADS) tile[k] = __fadd_rn(pre_root, t.uni_logp[t0 + k]);
    for (int j = levels - 2; j >= 0; --j) {     // shallow to deep: the deeper level must win
      __syncthreads();
      const float pre = sh_pre[j];
      for (int e = sh_a[j] + tid; e < sh_b[j]; e += NG_THREADS) {
        const int k = t.succ_label[e] - t0;
        if (k >= 0 && k < len) tile[k] = __fadd_rn(pre, t.succ_logp[e]);
      }
    }
  } else {
    for (int k = tid; k < len; k += NG_THREADS) tile[k] = __builtin_nanf("");
  }
  __syncthreads();
  // ---- write the tile out: 16-byte stores over the aligned middle of the row's part, scalar stores at its ends
  const long base = (long)r * t.V + t0;
  {
    float* dst = lp_out + base;
    const int head = min(len, (int)((4 - (((uintptr_t)dst >> 2) & 3)) & 3));
    const int nvec = (len - head) >> 2;
    if (tid < head) dst[tid] = tile[tid];
    for (int q = tid; q < nvec; q += NG_THREADS) {
      const int k = head + 4 * q;
      *reinterpret_cast<f32x4*>(dst + k) = f32x4{tile[k], tile[k + 1], tile[k + 2], tile[k + 3]};
    }
    for (int k = head + 4 * nvec + tid; k < len; k += NG_THREADS) dst[k] = tile[k];
  }
  if (comb_out) {                               // att + lm_weight * lp: the product, then the sum, each rounded to fp32 (add_scaled: no fma)
    float* dst = comb_out + base;
    const float* a = att + base;
    const int mis = (int)(((uintptr_t)dst >> 2) & 3);
    if (mis == (int)(((uintptr_t)a >> 2) & 3)) {
      const int head = min(len, (4 - mis) & 3);
      const int nvec = (len - head) >> 2;
      if (tid < head) dst[tid] = add_scaled(a[tid], lm_weight, tile[tid]);
      for (int q = tid; q < nvec; q += NG_THREADS) {
        const int k = head + 4 * q;
        const f32x4 av = *reinterpret_cast<const f32x4*>(a + k);
        *reinterpret_cast<f32x4*>(dst + k) = f32x4{add_scaled(av.x, lm_weight, tile[k]), add_scaled(av.y, lm_weight, tile[k + 1]),
                                                   add_scaled(av.z, lm_weight, tile[k + 2]), add_scaled(av.w, lm_weight, tile[k + 3])};
      }
      for (int k = head + 4 * nvec + tid; k < len; k += NG_THREADS) dst[k] = add_scaled(a[k], lm_weight, tile[k]);
    } else {
      for (int k = tid; k < len; k += NG_THREADS) dst[k] = add_scaled(a[k], lm_weight, tile[k]);
    }
  }
}

__global__ __launch_bounds__(64) void ngram_score_seqs_kernel(NgTables t, const int* __restrict__ labels, int Lmax, const int* __restrict__ lens, int S,
                                                              int eos, int append_eos, double* __restrict__ total_out) {
  const int q = blockIdx.x * 64 + threadIdx.x;
  if (q >= S) return;
  const int L = lens[q];
  bool ok = L >= 0 && L <= Lmax;
  int node = 0;
  if (ok) {
    node = t.uni_next[eos];                     // the context [eos]
    ok = node >= 0 && node < t.N;
  }
  double total = 0.0;
  const int steps = ok ? L + (append_eos ? 1 : 0) : 0;
  for (int p = 0; p < steps && ok; ++p) {       // ascending positions
    const int xr = p < L ? labels[(long)q * Lmax + p] : eos;
    float term;
    int next;
    ok = xr >= 0 && xr < t.V && ng_walk(t, node, xr, term, next);
    if (ok) {
      total += (double)term;
      node = next;
    }
  }
  total_out[q] = ok ? total : (double)__builtin_nanf("");
}

}  // namespace

#define NG_CHECK_TABLES()                                                                                                                \
  RE2E_CHECK_ARG(uni_logp && uni_next && bo && bo_node && succ_off && succ_label && succ_logp && succ_next, "null table");                \
  RE2E_CHECK_ARG(N > 0 && nsucc >= 0 && V > 0 && order >= 1 && order <= NG_MAXLEV, "bad shape (orders 1 .. 8)")

extern "C" int re2e_ngram_step(const float* uni_logp, const int* uni_next, const float* bo, const int* bo_node, const int* succ_off,
                               const int* succ_label, const float* succ_logp, const int* succ_next, int N, int nsucc, int V, int order,
                               const int* state_in, const int* x, int n, const float* att, float lm_weight, int* state_out, float* lp_out,
                               float* comb_out, hipStream_t stream) {
  NG_CHECK_TABLES();
  RE2E_CHECK_ARG(x && state_out && lp_out, "null operand");
  RE2E_CHECK_ARG(n > 0, "bad shape");
  RE2E_CHECK_ARG((att != nullptr) == (comb_out != nullptr), "att and comb_out go together");
  RE2E_CHECK_ARG(comb_out != lp_out, "comb_out must not alias lp_out");
  const int tiles = cdiv(V, NG_TILE);
  RE2E_CHECK_ARG((long)n * tiles <= 0x7fffffffL, "too many rows for one launch");
  const NgTables t{uni_logp, uni_next, bo, bo_node, succ_off, succ_label, succ_logp, succ_next, N, nsucc, V};
  hipLaunchKernelGGL(ngram_step_kernel, dim3((unsigned)((long)n * tiles)), dim3(NG_THREADS), 0, stream, t, state_in, x, tiles, att, lm_weight,
                     state_out, lp_out, comb_out);
  RE2E_LAUNCH_CHECK();
  return RE2E_OK;
}

extern "C" int re2e_ngram_score_seqs(const float* uni_logp, const int* uni_next, const float* bo, const int* bo_node, const int* succ_off,
                                     const int* succ_label, const float* succ_logp, const int* succ_next, int N, int nsucc, int V, int order,
                                     const int* labels, int Lmax, const int* lens, int S, int eos, int append_eos, double* total_out,
                                     hipStream_t stream) {
  NG_CHECK_TABLES();
  RE2E_CHECK_ARG(labels && lens && total_out, "null operand");
  RE2E_CHECK_ARG(S > 0 && Lmax >= 0 && eos >= 0 && eos < V, "bad shape");
  const NgTables t{uni_logp, uni_next, bo, bo_node, succ_off, succ_label, succ_logp, succ_next, N, nsucc, V};
  hipLaunchKernelGGL(ngram_score_seqs_kernel, dim3(cdiv(S, 64)), dim3(64), 0, stream, t, labels, Lmax, lens, S, eos, append_eos, total_out);
  RE2E_LAUNCH_CHECK();
  return RE2E_OK;
}
