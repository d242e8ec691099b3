// K12 scoring: weighted edit-distance alignment of many pairs of integer label sequences in one launch.
//
// Definition (include/re2e.h, re2e_align_counts): D[i][0] = i deletions, D[0][j] = j insertions, cell (i, j) takes the smallest
// (cost, errors) pair, compared lexicographically, of  diagonal (match at 0 / substitution at c_sub), deletion from (i-1, j), insertion from
// (i, j-1) -- on a full tie the earlier of the three.  Everything is integer: a cell is ONE 32-bit key, cost << 12 | errors (costs <= 255 and
// lengths <= 1024 keep cost < 2^19 and errors < 2^12, candidates included), so "smaller pair" is "smaller key" and adding a step is one
// integer addition.  A second word carries the substitutions and deletions of the cell's own path (S << 16 | D): the counts come out of the
// forward sweep, C = |ref| - S - D and I = errors - S - D, and a call without paths writes no choice bits and walks nothing back.
//
// One wavefront per pair, four pairs per workgroup, no wave waits on another.  Lane l owns reference row i0 + l + 1 of a strip of 64 rows and
// sweeps the anti-diagonals: at step s it fills column j = s - l.  What it needs of row i - 1 is what the lane below held one step ago (the
// cell above) and two steps ago (the diagonal one), a one-lane shift of the wavefront (DPP wave_shr:1); the hypothesis label of a column
// travels up the lanes the same way.  Lane 0 takes all three from the strip's boundary row instead (row i0: the j insertions of row 0, or
// what lane 63 of the strip before wrote), kept in LDS in two buffers that swap per strip, read 64 columns at a time and handed to lane 0 by
// v_readlane.  With paths, a lane packs its choices (2 bits a cell) sixteen to a word into the caller's workspace and lane 0 walks back from
// (|ref|, |hyp|) once the sweep is done, writing the path from its end.
#include <vector>

#include "common.h"

namespace {

constexpr int ALIGN_WAVES = 4;          // pairs per workgroup
constexpr int ALIGN_MAX_LEN = 1024;     // labels per sequence
constexpr int ALIGN_MAX_COST = 255;
constexpr int ERR_BITS = 12;

__device__ __forceinline__ unsigned wave_shr1(unsigned v) {      // lane l <- lane l - 1; lane 0 <- 0.  Called with all 64 lanes active.
  return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x138, 0xf, 0xf, false);
}
__device__ __forceinline__ unsigned from_lane(unsigned v, int lane) {      // lane: wave-uniform
  return (unsigned)__builtin_amdgcn_readlane((int)v, lane);
}
__device__ __forceinline__ void wave_publish() {      // one wave's LDS / global writes before its own later reads from other lanes
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

template <bool PATH>
__global__ __launch_bounds__(64 * ALIGN_WAVES) void align_kernel(const int* __restrict__ ref_labels, const int* __restrict__ hyp_labels,
                                                                 const int* __restrict__ ref_off, const int* __restrict__ hyp_off,
                                                                 const int* __restrict__ pair_ref, int n_pairs, unsigned add_sub, unsigned add_ins,
                                                                 unsigned add_del, int ldb, int* __restrict__ counts, unsigned char* path,
                                                                 const long* __restrict__ path_off, unsigned* choice, const long* __restrict__ ws_off) {
  extern __shared__ uint2 align_lds[];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int n = blockIdx.x * ALIGN_WAVES + wid;
  if (n >= n_pairs) return;                 // the whole wave
  const int r = pair_ref[n];
  const int* ref = ref_labels + ref_off[r];
  const int R = ref_off[r + 1] - ref_off[r];
  const int* hyp = hyp_labels + hyp_off[n];
  const int H = hyp_off[n + 1] - hyp_off[n];
  uint2* bin = align_lds + (long)wid * 2 * ldb;      // ldb >= H + 1 (host)
  uint2* bout = bin + ldb;
  const int wpr = (H + 15) >> 4;                     // choice words per reference row
  unsigned* cw = PATH ? choice + ws_off[n] : nullptr;

  unsigned res_k = (unsigned)H * add_ins, res_sd = 0;      // |ref| == 0
  for (int j = lane; j <= H; j += 64) bin[j] = make_uint2((unsigned)j * add_ins, 0u);
  wave_publish();
  for (int i0 = 0; i0 < R; i0 += 64) {
    const int i = i0 + lane + 1;
    const bool row = i <= R;
    const int nl = R - i0 < 64 ? R - i0 : 64;
    const int rl = row ? ref[i - 1] : 0;
    unsigned pk = 0, psd = 0, dk = 0, dsd = 0, hl = 0, bits = 0, bck = 0, bcsd = 0, bch = 0;
    const int nsteps = H + nl;
    for (int s = 0; s < nsteps; ++s) {
      if ((s & 63) == 0) {                 // the boundary row and the labels of columns s .. s + 63, one per lane
        const int jj = s + lane;
        const uint2 b = jj <= H ? bin[jj] : make_uint2(0u, 0u);
        bck = b.x; bcsd = b.y;
        bch = (jj >= 1 && jj <= H) ? (unsigned)hyp[jj - 1] : 0u;
      }
      unsigned uk = wave_shr1(pk), usd = wave_shr1(psd), hj = wave_shr1(hl);
      const int q = s & 63;
      const unsigned b_k = from_lane(bck, q), b_sd = from_lane(bcsd, q), b_h = from_lane(bch, q);
      if (lane == 0) { uk = b_k; usd = b_sd; hj = b_h; }
      const int j = s - lane;
      if (row && j >= 0 && j <= H) {
        unsigned k, sd;
        if (j == 0) {
          k = (unsigned)i * add_del; sd = (unsigned)i;
        } else {
          const bool eq = rl == (int)hj;
          unsigned ch = eq ? 0u : 1u;
          k = dk + (eq ? 0u : add_sub); sd = dsd + (eq ? 0u : 0x10000u);
          unsigned t = uk + add_del;
          if (t < k) { k = t; sd = usd + 1u; ch = 2u; }
          t = pk + add_ins;
          if (t < k) { k = t; sd = psd; ch = 3u; }
          if (PATH) {
            bits |= ch << (2 * ((j - 1) & 15));
            if ((j & 15) == 0 || j == H) { cw[(long)(i - 1) * wpr + ((j - 1) >> 4)] = bits; bits = 0; }
          }
        }
        pk = k; psd = sd;
        if (lane == 63) bout[j] = make_uint2(k, sd);
      }
      dk = uk; dsd = usd; hl = hj;
    }
    res_k = from_lane(pk, nl - 1); res_sd = from_lane(psd, nl - 1);
    uint2* t = bin; bin = bout; bout = t;
    wave_publish();
  }

  const int cost = (int)(res_k >> ERR_BITS), err = (int)(res_k & ((1u << ERR_BITS) - 1u));
  const int S = (int)(res_sd >> 16), D = (int)(res_sd & 0xffffu);
  const int I = err - S - D, C = R - S - D;
  if (lane < 6) counts[(long)n * 6 + lane] = lane == 0 ? cost : lane == 1 ? err : lane == 2 ? C : lane == 3 ? S : lane == 4 ? D : I;
  if (PATH) {
    unsigned char* out = path + path_off[n];
    const long cap = path_off[n + 1] - path_off[n];      // >= R + H (host)
    const int P = R + I;                                 // C + S + D + I steps
    if (lane == 0) {
      int i = R, j = H, p = P;
      while ((i > 0 || j > 0) && p > 0) {                // every trip lowers i or j: at most R + H trips
        const unsigned ch = i == 0 ? 3u : j == 0 ? 2u : (cw[(long)(i - 1) * wpr + ((j - 1) >> 4)] >> (2 * ((j - 1) & 15))) & 3u;
        out[--p] = ch == 0u ? 'C' : ch == 1u ? 'S' : ch == 2u ? 'D' : 'I';
        if (ch != 3u) --i;
        if (ch != 2u) --j;
      }
    }
    for (long p = P + lane; p < cap; p += 64) out[p] = 0;
  }
}

// The device copy of the tables, at the head of the workspace: ws_off[n_pairs] and path_off[n_pairs + 1] (long), then ref_off[n_ref + 1],
// hyp_off[n_pairs + 1], pair_ref[n_pairs] (int), padded to 16 bytes; the choice words follow.
struct Layout { size_t ws_off, path_off, ref_off, hyp_off, pair_ref, tables, total; };

Layout layout_of(int n_ref, int n_pairs, long choice_words) {
  Layout l;
  l.ws_off = 0;
  l.path_off = l.ws_off + sizeof(long) * (size_t)n_pairs;
  l.ref_off = l.path_off + sizeof(long) * ((size_t)n_pairs + 1);
  l.hyp_off = l.ref_off + sizeof(int) * ((size_t)n_ref + 1);
  l.pair_ref = l.hyp_off + sizeof(int) * ((size_t)n_pairs + 1);
  l.tables = (l.pair_ref + sizeof(int) * (size_t)n_pairs + 15) & ~(size_t)15;
  l.total = l.tables + sizeof(unsigned) * (size_t)choice_words;
  return l;
}

// Everything the kernel will trust, checked on the host.  0, or the error code with the message set.  Fills the choice-word offsets (when asked
// for) and the longest hypothesis.
int check_tables(const char* who, const int* ref_off, int n_ref, long n_ref_labels, const int* hyp_off, const int* pair_ref, int n_pairs,
                 long n_hyp_labels, std::vector<long>* ws_off, long* choice_words, int* h_max) {
  if (!ref_off || !hyp_off || !pair_ref || n_ref < 1 || n_pairs < 1) { re2e_set_error("%s: null table or no pairs", who); return RE2E_EINVAL; }
  if (ref_off[0] < 0 || hyp_off[0] < 0) { re2e_set_error("%s: an offset table starts below 0", who); return RE2E_EINVAL; }
  for (int r = 0; r < n_ref; ++r) {
    if (ref_off[r + 1] < ref_off[r]) { re2e_set_error("%s: ref_off decreases at %d (%d after %d)", who, r + 1, ref_off[r + 1], ref_off[r]); return RE2E_EINVAL; }
  }
  if (n_ref_labels >= 0 && ref_off[n_ref] > n_ref_labels) { re2e_set_error("%s: ref_off ends at %d, beyond the %ld labels given", who, ref_off[n_ref], n_ref_labels); return RE2E_EINVAL; }
  long words = 0;
  int hm = 0;
  if (ws_off) ws_off->resize(n_pairs);
  for (int n = 0; n < n_pairs; ++n) {
    if (hyp_off[n + 1] < hyp_off[n]) { re2e_set_error("%s: hyp_off decreases at %d (%d after %d)", who, n + 1, hyp_off[n + 1], hyp_off[n]); return RE2E_EINVAL; }
    if (pair_ref[n] < 0 || pair_ref[n] >= n_ref) { re2e_set_error("%s: pair_ref[%d] = %d is not one of the %d references", who, n, pair_ref[n], n_ref); return RE2E_EINVAL; }
    const int R = ref_off[pair_ref[n] + 1] - ref_off[pair_ref[n]], H = hyp_off[n + 1] - hyp_off[n];
    if (R > ALIGN_MAX_LEN || H > ALIGN_MAX_LEN) {
      re2e_set_error("%s: pair %d has %d reference and %d hypothesis labels; at most %d per sequence are supported", who, n, R, H, ALIGN_MAX_LEN);
      return RE2E_EUNSUPPORTED;
    }
    if (ws_off) (*ws_off)[n] = words;
    words += (long)R * ((H + 15) >> 4);
    if (H > hm) hm = H;
  }
  if (n_hyp_labels >= 0 && hyp_off[n_pairs] > n_hyp_labels) { re2e_set_error("%s: hyp_off ends at %d, beyond the %ld labels given", who, hyp_off[n_pairs], n_hyp_labels); return RE2E_EINVAL; }
  if (choice_words) *choice_words = words;
  if (h_max) *h_max = hm;
  return RE2E_OK;
}

LdsLimit g_lds_counts, g_lds_path;

}  // namespace

extern "C" size_t re2e_align_counts_workspace_bytes(const int* ref_off_host, int n_ref, const int* hyp_off_host, const int* pair_ref_host, int n_pairs,
                                                    int with_path) {
  long words = 0;
  if (check_tables(__func__, ref_off_host, n_ref, -1, hyp_off_host, pair_ref_host, n_pairs, -1, nullptr, &words, nullptr) != RE2E_OK) return 0;
  return layout_of(n_ref, n_pairs, with_path ? words : 0).total;
}

extern "C" int re2e_align_counts(const int* ref_labels, const int* ref_off_host, int n_ref, long n_ref_labels, const int* hyp_labels,
                                 const int* hyp_off_host, const int* pair_ref_host, int n_pairs, long n_hyp_labels, int c_sub, int c_ins, int c_del,
                                 int* counts, unsigned char* path, const long* path_off_host, long path_bytes, void* workspace,
                                 size_t workspace_bytes, hipStream_t stream) {
  RE2E_CHECK_ARG(counts && workspace, "null operand");
  RE2E_CHECK_ARG(n_ref_labels >= 0 && n_hyp_labels >= 0, "negative label count");
  RE2E_CHECK_ARG((ref_labels || n_ref_labels == 0) && (hyp_labels || n_hyp_labels == 0), "null label array");
  RE2E_CHECK_ARG(c_sub >= 1 && c_sub <= ALIGN_MAX_COST && c_ins >= 1 && c_ins <= ALIGN_MAX_COST && c_del >= 1 && c_del <= ALIGN_MAX_COST,
                 "costs must be integers in 1 .. 255");
  RE2E_CHECK_ARG((path == nullptr) == (path_off_host == nullptr), "path and path_off_host go together");
  std::vector<long> ws_off;
  long words = 0;
  int h_max = 0;
  const int rc = check_tables(__func__, ref_off_host, n_ref, n_ref_labels, hyp_off_host, pair_ref_host, n_pairs, n_hyp_labels, &ws_off, &words, &h_max);
  if (rc != RE2E_OK) return rc;
  if (path) {
    RE2E_CHECK_ARG(path_off_host[0] >= 0, "path_off starts below 0");
    for (int n = 0; n < n_pairs; ++n) {
      const long need = (long)(ref_off_host[pair_ref_host[n] + 1] - ref_off_host[pair_ref_host[n]]) + (hyp_off_host[n + 1] - hyp_off_host[n]);
      if (path_off_host[n + 1] - path_off_host[n] < need) {
        re2e_set_error("%s: path_off leaves %ld bytes for pair %d, which may take %ld", __func__, path_off_host[n + 1] - path_off_host[n], n, need);
        return RE2E_EINVAL;
      }
    }
    RE2E_CHECK_ARG(path_off_host[n_pairs] <= path_bytes, "path_off ends beyond the path buffer");
  }
  const Layout l = layout_of(n_ref, n_pairs, path ? words : 0);
  if (workspace_bytes < l.total) { re2e_set_error("%s: workspace of %zu bytes, %zu needed", __func__, workspace_bytes, l.total); return RE2E_EINVAL; }
  RE2E_CHECK_ARG(((uintptr_t)workspace & 15) == 0, "workspace must be 16-byte aligned");

  std::vector<unsigned char> host(l.tables, 0);
  memcpy(host.data() + l.ws_off, ws_off.data(), sizeof(long) * (size_t)n_pairs);
  if (path) memcpy(host.data() + l.path_off, path_off_host, sizeof(long) * ((size_t)n_pairs + 1));
  memcpy(host.data() + l.ref_off, ref_off_host, sizeof(int) * ((size_t)n_ref + 1));
  memcpy(host.data() + l.hyp_off, hyp_off_host, sizeof(int) * ((size_t)n_pairs + 1));
  memcpy(host.data() + l.pair_ref, pair_ref_host, sizeof(int) * (size_t)n_pairs);
  // the staging vector dies with this call: the upload has to be over before it does
  hipError_t e = hipMemcpyAsync(workspace, host.data(), l.tables, hipMemcpyHostToDevice, stream);
  if (e == hipSuccess) e = hipStreamSynchronize(stream);
  if (e != hipSuccess) { re2e_set_error("%s: table upload failed: %s", __func__, hipGetErrorString(e)); return RE2E_EHIP; }

  unsigned char* w = (unsigned char*)workspace;
  const int ldb = h_max + 1;
  const size_t lds = sizeof(uint2) * 2 * (size_t)ldb * ALIGN_WAVES;      // <= 65600 bytes
  const unsigned add_sub = ((unsigned)c_sub << ERR_BITS) | 1u, add_ins = ((unsigned)c_ins << ERR_BITS) | 1u, add_del = ((unsigned)c_del << ERR_BITS) | 1u;
  const dim3 grid(cdiv(n_pairs, ALIGN_WAVES)), block(64 * ALIGN_WAVES);
  if (path) {
    g_lds_path.ensure((const void*)align_kernel<true>, lds);
    hipLaunchKernelGGL(align_kernel<true>, grid, block, lds, stream, ref_labels, hyp_labels, (const int*)(w + l.ref_off), (const int*)(w + l.hyp_off),
                       (const int*)(w + l.pair_ref), n_pairs, add_sub, add_ins, add_del, ldb, counts, path, (const long*)(w + l.path_off),
                       (unsigned*)(w + l.tables), (const long*)(w + l.ws_off));
  } else {
    g_lds_counts.ensure((const void*)align_kernel<false>, lds);
    hipLaunchKernelGGL(align_kernel<false>, grid, block, lds, stream, ref_labels, hyp_labels, (const int*)(w + l.ref_off), (const int*)(w + l.hyp_off),
                       (const int*)(w + l.pair_ref), n_pairs, add_sub, add_ins, add_del, ldb, counts, (unsigned char*)nullptr, (const long*)nullptr,
                       (unsigned*)nullptr, (const long*)nullptr);
  }
  RE2E_LAUNCH_CHECK();
  return RE2E_OK;
}
