// N3: beam pruning on the device for a search over several utterances (model/beam_search.py recognize_beam_batch).
//
// The rows of a position are the live hypotheses of all unfinished utterances, grouped by utterance (seg_off).  Every row has `ncand`
// scored continuations, local[row][col]; an utterance keeps the `beam` best of rows x ncand by score = hyp_score[row] + local[row][col].
// The host loop this replaces (recognize_beam: per hypothesis the top `beam` of its local scores, appended to a list that is stably
// re-sorted by score and cut to `beam` after every hypothesis) orders the survivors by
//     score descending, then parent row ascending, then local descending, then column ascending
// (the third key is not implied by the first: fp32 rounding can give two different locals of one hypothesis the same sum, and the host
// keeps the larger local first whatever its column).  fl(h + x) is non-decreasing in x, so within a row that order is (local descending,
// column ascending) and the survivors of an utterance are among the first `beam` of each of its rows in that order.  Two launches:
//   beam_row_topk (one workgroup per row)      : the row's first min(beam, ncand) entries, block_topk256 over the row held in LDS
//   beam_merge    (one wavefront per utterance): lane = row of the utterance, a head index into its sorted list; `beam` rounds of a
//                                                wavefront arg-max over the heads' sums (ties -> lower row), the winner advances
// The (rows, ncand) scores never leave the device; four (U, beam) arrays and U counts do.
// NaN: a NaN local ranks as -inf within its row and a NaN sum as -inf between rows, as in the CTC prefix kernel's selection (torch / numpy
// would rank it first); the score written is the sum itself.  Inputs that are finite or -inf give exactly the host loop's list.
#include "common.h"

namespace {
constexpr int PRUNE_MAX_BEAM = 64;

__global__ __launch_bounds__(256) void beam_row_topk_kernel(const float* __restrict__ local, int ncand, int kk, float* __restrict__ top_val,
                                                            int* __restrict__ top_col) {
  extern __shared__ float row[];         // [ncand]
  __shared__ float red_v[4];
  __shared__ int red_i[4];
  __shared__ int sel_i[PRUNE_MAX_BEAM];
  __shared__ float sel_v[PRUNE_MAX_BEAM];
  const int h = blockIdx.x, tid = threadIdx.x;
  for (int i = tid; i < ncand; i += 256) { const float v = local[(long)h * ncand + i]; row[i] = v == v ? v : -INFINITY; }
  __syncthreads();
  block_topk256(row, ncand, kk, sel_i, sel_v, red_v, red_i);      // kk <= ncand
  if (tid < kk) {
    const int c = sel_i[tid];
    top_col[(long)h * kk + tid] = c;
    top_val[(long)h * kk + tid] = local[(long)h * ncand + c];      // the value itself (a NaN stays one: the sum below is the caller's score)
  }
}

__global__ __launch_bounds__(64) void beam_merge_kernel(const int* __restrict__ seg_off, const float* __restrict__ hyp_score, const float* __restrict__ top_val,
                                                        const int* __restrict__ top_col, const int* __restrict__ cand, int nh, int ncand, int kk, int beam,
                                                        int* __restrict__ parent_out, int* __restrict__ col_out, int* __restrict__ label_out,
                                                        float* __restrict__ score_out, int* __restrict__ count_out) {
  constexpr int NONE = 0x7fffffff;
  const int u = blockIdx.x, lane = threadIdx.x;
  const int r0 = min(max(seg_off[u], 0), nh), r1 = min(max(seg_off[u + 1], r0), nh);     // a bad offset must not become an address
  const int nrows = min(r1 - r0, PRUNE_MAX_BEAM);
  const int total = min(beam, nrows * kk);
  const bool on = lane < nrows;
  const int row = r0 + lane;
  const float hs = on ? hyp_score[row] : 0.f;
  int head = 0;
  for (int k = 0; k < beam; ++k) {
    const long o = (long)u * beam + k;
    if (k >= total) {                    // (uniform) fewer continuations than `beam`: the tail is defined
      if (lane == 0) { parent_out[o] = -1; col_out[o] = -1; label_out[o] = -1; score_out[o] = -INFINITY; }
      continue;
    }
    const bool has = on && head < kk;
    const float s = has ? __fadd_rn(hs, top_val[(long)row * kk + head]) : 0.f;
    float bv = has ? (s == s ? s : -INFINITY) : -INFINITY;
    int bi = has ? lane : NONE;
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
      const float ov = __shfl_xor(bv, d, 64); const int oi = __shfl_xor(bi, d, 64);
      if (oi != NONE && (bi == NONE || ov > bv || (ov == bv && oi < bi))) { bv = ov; bi = oi; }
    }
    if (lane == bi) {                    // k < total: a head is left, bi is a lane
      const int c = top_col[(long)row * kk + head];
      parent_out[o] = row; col_out[o] = c; label_out[o] = cand ? cand[(long)row * ncand + c] : c; score_out[o] = s;
      ++head;
    }
  }
  if (lane == 0) count_out[u] = total;
}
}  // namespace

extern "C" int re2e_beam_prune(const int* seg_off_dev, int U, int max_seg_rows, const float* hyp_score, const float* local, const int* cand_dev, int nh,
                               int ncand, int beam, int* parent_out, int* col_out, int* label_out, float* score_out, int* count_out, void* workspace,
                               size_t workspace_bytes, hipStream_t stream) {
  RE2E_CHECK_ARG(seg_off_dev && hyp_score && local && parent_out && col_out && label_out && score_out && count_out && workspace, "null operand");
  RE2E_CHECK_ARG(U > 0 && nh > 0 && ncand > 0 && beam > 0 && max_seg_rows > 0 && max_seg_rows <= nh, "bad geometry");
  if (beam > PRUNE_MAX_BEAM || max_seg_rows > beam) {
    re2e_set_error("re2e_beam_prune: beam <= %d and at most `beam` rows per utterance (got beam %d, %d rows)", PRUNE_MAX_BEAM, beam, max_seg_rows);
    return RE2E_EUNSUPPORTED;
  }
  const int kk = beam < ncand ? beam : ncand;
  RE2E_CHECK_ARG(workspace_bytes >= (size_t)2 * nh * kk * sizeof(float), "workspace too small (2 * nh * min(beam, ncand) words)");
  const size_t lds = (size_t)ncand * sizeof(float);
  if (lds > 150 * 1024) { re2e_set_error("re2e_beam_prune: ncand floats exceed the LDS"); return RE2E_EUNSUPPORTED; }
  float* top_val = (float*)workspace;
  int* top_col = (int*)workspace + (size_t)nh * kk;
  static LdsLimit lim;
  lim.ensure(reinterpret_cast<const void*>(&beam_row_topk_kernel), lds);
  hipLaunchKernelGGL(beam_row_topk_kernel, dim3(nh), dim3(256), lds, stream, local, ncand, kk, top_val, top_col);
  hipLaunchKernelGGL(beam_merge_kernel, dim3(U), dim3(64), 0, stream, seg_off_dev, hyp_score, (const float*)top_val, (const int*)top_col, cand_dev, nh, ncand,
                     kk, beam, parent_out, col_out, label_out, score_out, count_out);
  RE2E_LAUNCH_CHECK();
  return RE2E_OK;
}
