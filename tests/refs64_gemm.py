"""Float64 reference of the dense products at their C-ABI contract (re2e_gemm, re2e_gemm_nt_rows, re2e_gemm_tn_rows, re2e_gemm_skinny2:
include/re2e.h; csrc/igemm.hip's engine and skinny kernels, csrc/gemm_nt.hip's LDS-DMA pipeline with its stream-K tail) and the inputs of
tests/test_dense_kernels_gpu.py.

Plain torch on the CPU, nothing imported from the product or from ``oracle``.  ``dense_ref`` is written from the header's contract:
C = act(op(A) op(B) + bias + bias2) + beta C0 (the activation BEFORE the beta term), the mask epilogue, the row maps of both mapped entry
points, leading dimensions larger than the widths; tests/test_refs64_gemm_cpu.py pins it to F.linear / @ / index_select / index_add on
doubles.  Like the references of tests/refs64.py it takes ``dtype``: float64 is the truth, the SAME code in float32 -- the sum over k written
out (refs64_conv._mm; ``order='k2'``: strictly in k-steps of 2, slice by slice) -- says how far fp32 arithmetic alone is from it.

``DENSE_CASES`` holds one row per kernel form the plan (re2e_gemm_plan: csrc/igemm.hip plan_gemm) can name on a 256-CU chip, keyed by
``form_key``, plus the two forms below the plan (the pipeline's run-time fallback to the engine, re2e_gemm_skinny2);
tests/test_refs64_gemm_cpu.py checks that the table is closed under a sweep of the plans.  ``EDGES`` turns the tile, k-tile, alignment, row-map
and mask boundaries of each family.  The K-sliced batches (gemm_kslices, gemm_kslices_tn) have no C entry point of their own: they are
covered through the F(2x2,4x4) rows of tests/test_conv_kernels_gpu.py and left out here.  The mask epilogue is swept and run on all three operand forms:
re2e_gemm takes it in every form (ops.py asks for it on the enhancer's x W^T alone); its rows are the (b, t) frames of the OUTPUT.

Every input here is finite.  What the same forms make of a NaN or an infinity in A is tests/refs64_nonfinite.py's subject (poison_dense).
"""
import collections
import math

import torch

from refs64 import rel_err, rnd          # noqa: F401  (re-exported: the dense tests use them through this module)
from refs64_conv import _mm, round11     # noqa: F401

ACT_NONE, ACT_TANH, ACT_RELU, ACT_LRELU, ACT_SIGMOID, ACT_MASK = range(6)          # include/re2e.h RE2E_ACT_*
OPS = {(0, 1): 'nt', (0, 0): 'nn', (1, 0): 'tn'}          # (transa, transb): x W^T, x W, x^T W
TRANS = {v: k for k, v in OPS.items()}

# deliberate mistakes the sensitivity test applies to the reference (never used for a yardstick)
MISTAKES = {
    'a': 'the last k dropped',
    'b': 'the last output row computed from the row before it',
    'c': 'the last four columns left out',
    'd': 'one K slice (of a split) or one 16-k unit (of a cut tile) dropped',
    'e': 'bias2 ignored',
    'f': 'beta ignored',
    'g': 'the activation applied after the beta term',
    'h': 'a row-map entry off by one',
    'i': 'the mask epilogue\'s length test taken as <=',
    'j': 'both operands rounded to 11 mantissa bits',
    'k': 'both operands rounded to 16 mantissa bits (a two-term bf16 split)',
}


def round16(t):
    """Every element rounded to 16 mantissa bits behind the leading one: what the sum of two bf16 terms carries (mistake 'k')."""
    m, e = torch.frexp(t.double())
    return torch.ldexp(torch.round(m * 131072.0) / 131072.0, e).to(t.dtype)


def _mm_k2(a, b, slices):
    """a (P,K) @ b (K,N) in float32, accumulated strictly in k-steps of 2 (the step of mfma_f32_32x32x2f32: acc += a0 b0 + a1 b1), every K slice
    summed on its own from zero and the slices then added in slice order.  Elementwise operations alone, like _mm."""
    assert a.dtype == torch.float32
    K = a.shape[1]
    total = None
    for k0, k1 in slices:
        acc = torch.zeros(a.shape[0], b.shape[1], dtype=a.dtype)
        for k in range(k0, k1, 2):
            t = a[:, k, None] * b[None, k, :]
            if k + 1 < k1:
                t = t + a[:, k + 1, None] * b[None, k + 1, :]
            acc += t
        total = acc if total is None else total + acc
    assert sum(k1 - k0 for k0, k1 in slices) == K
    return total


# ---------------------------------------------------------------------------------------------
# rows
# ---------------------------------------------------------------------------------------------
# form: the plan's form_key (None: an edge, it runs whatever the plan names); op: 'nt' / 'nn' / 'tn'; M, N, K: the LOGICAL sizes (mapped entry
# points: M = Mv of re2e_gemm_nt_rows, K = Kv of re2e_gemm_tn_rows); bias / bias2 / beta: 0 or 1; pad: what lda, ldb, ldc exceed the widths by;
# off: floats the base pointers of A, B, C sit behind a 16-byte boundary; entry: 'gemm', 'gemm_nows' (re2e_gemm with a NULL workspace: the
# pipeline's run-time fallback), 'nt_rows', 'tn_rows', 'skinny2' (N = N1 + N2, n1 = N1); rmap: (identity prefix, ident_rows passed, descending,
# physical rows behind the last mapped one); T, lens: the mask epilogue's frames per utterance and lengths (M = len(lens) * T); plan: the plan the
# row declares (strings, as re2e_gemm_plan prints them), alignment and stream role taken from the row.
Row = collections.namedtuple('Row', 'form op M N K act bias bias2 beta pad off filler entry rmap T lens n1 plan')
Query = collections.namedtuple('Query', 'op M K act entry')          # what form_key needs of a sweep point


def _row(form, op, M, N, K, act=ACT_NONE, bias=1, bias2=0, beta=0, pad=(4, 8, 4), off=(0, 0, 0), filler=False, entry='gemm', rmap=None, T=0, lens=None,
         n1=0, plan=None):
    if entry in ('tn_rows', 'skinny2'):
        bias = bias2 = 0          # (re2e_gemm_tn_rows and re2e_gemm_skinny2 take no bias; re2e_gemm takes both in every operand form, x^T W included)
    return Row(form, op, M, N, K, act, bias, bias2, beta, pad, off, filler, entry, rmap, T, lens, n1, plan)


def widths(row):
    """(columns of A, of B, of C) as stored."""
    return (row.M if row.op == 'tn' else row.K, row.K if row.op == 'nt' else row.N, row.N)


def leading_dims(row):
    return tuple(w + p for w, p in zip(widths(row), row.pad))


def aligned_of(row):
    """(a16, b16, c16) as the entry points derive them: a 16-byte aligned base and a leading dimension of whole float4s."""
    return tuple(o == 0 and ld % 4 == 0 for o, ld in zip(row.off, leading_dims(row)))


def plan_args(row):
    """The arguments of lib.gemm_plan for a row (cus aside).  re2e_gemm_nt_rows takes one alignment flag for all three operands."""
    al = aligned_of(row)
    if row.entry == 'nt_rows':
        al = (all(al),) * 3
    if row.entry == 'gemm_nows':
        al = (al[0], al[1], False)          # the engine plan the fallback lands on: the same product with the pipeline out of reach
    ta, tb = TRANS[row.op]
    return (ta, tb, row.M, row.N, row.K), dict(act=row.act, aligned=al, rowmap=row.entry in ('nt_rows', 'tn_rows'), filler=row.filler)


def form_key(plan, q):
    """The kernel form a re2e_gemm_plan answer (a dict of strings) names for a Row / Query, as DENSE_CASES writes it; None where the mapped entry
    point refuses instead of running the plan (re2e_gemm_nt_rows: not the pipeline; re2e_gemm_tn_rows: no 16-byte loads or Kv < 64).  The stream
    role is no part of it: it only selects among these forms."""
    mapped = q.entry in ('nt_rows', 'tn_rows')
    r = plan['route']
    if r == 'skinny_wg':
        return (r, q.op, int(plan['vec']))
    if r == 'pipeline':
        n_dp, g_sk = int(plan['n_dp']), int(plan['g_sk'])
        return (r, int(plan['variant']), 'dp' if g_sk == 0 else 'dp+sk' if n_dp > 0 else 'sk', int(mapped))
    assert r == 'engine'
    if mapped and (q.op != 'tn' or plan['vec'] != '1' or q.K < 64):
        return None
    s = int(plan['splits'])
    return (r, q.op, int(plan['vec']), plan['tile'], 'one' if s == 1 else 'zx' if s % 8 == 0 else 'split', int(int(plan['m1']) < q.M), int(q.act == ACT_MASK),
            int(mapped))


def family_of(row, plan):
    """The key of BARS a row is held to: the mask epilogue, the skinny kernels, the pipeline, the engine with one K slice or with several."""
    if row.act == ACT_MASK:
        fam = 'mask'
    elif row.entry == 'skinny2' or plan['route'] == 'skinny_wg':
        fam = 'skinny_wg'
    elif plan['route'] == 'pipeline':
        fam = 'pipeline'
    else:
        fam = 'engine_split' if int(plan['splits']) > 1 else 'engine'
    return fam, 'K<=1024' if row.K <= 1024 else 'K>1024'


def k_slices(row, plan):
    """The K ranges a plan sums on their own before they meet: the engine's split (igemm_kernel: ceil(k-tiles / splits) k-tiles per slice), the eight
    wavefronts of the skinny kernels (ceil(k-groups of 8 / 8) groups each); one range otherwise (a cut tile of the pipeline is summed in k order)."""
    K = row.K
    if row.entry == 'skinny2' or plan['route'] == 'skinny_wg':
        per = -(-(-(-K // 8)) // 8) * 8
    elif plan['route'] == 'engine' and int(plan['splits']) > 1:
        bk = int(plan['tile'].split('x')[2])
        per = -(-(-(-K // bk)) // int(plan['splits'])) * bk
    else:
        per = K
    return [(k0, min(K, k0 + per)) for k0 in range(0, K, per)]


def map_of(row):
    """-> (int64 map of the logical rows, physical rows) of a mapped row, from row.rmap = (i0, ident, desc, extra): rows [0, i0) map to themselves,
    the others to every second physical row from i0 + 1 on (so map[i0] != i0 and the identity prefix is exactly i0 long); desc: the whole map
    reversed; extra physical rows behind the last mapped one (0: the last entry is the last physical row)."""
    i0, ident, desc, extra = row.rmap
    n = row.M if row.entry == 'nt_rows' else row.K
    assert 0 <= ident <= i0 <= n and not (desc and ident)
    m = torch.cat([torch.arange(i0), i0 + 1 + 2 * torch.arange(n - i0)])
    phys = int(m.max()) + 1 + extra
    return (m.flip(0) if desc else m).contiguous(), phys


def dense_case(row):
    """The inputs of a row, a function of its shape: A and B as stored (mapped entry points: all physical rows, finite everywhere -- the GPU test
    puts NaN into the rows the map leaves out --), B ~ N(0, 1/K) so that the pre-activations are N(0, 1) and tanh / sigmoid do not saturate,
    b1, b2, the prior content C0 of C (physical rows x N), the mask epilogue's mul and the prior content of mask_out."""
    g = torch.Generator().manual_seed(row.M * 1000003 + row.N * 10007 + row.K * 101 + row.act * 7 + len(row.entry))
    M, N, K = row.M, row.N, row.K
    rmap, phys = map_of(row) if row.rmap is not None else (None, 0)
    s = K ** -0.5
    if row.op == 'nt':
        A, B = rnd(g, phys if row.entry == 'nt_rows' else M, K), rnd(g, N, K, scale=s)
    elif row.op == 'nn':
        A, B = rnd(g, M, K), rnd(g, K, N, scale=s)
    else:
        A, B = rnd(g, phys if row.entry == 'tn_rows' else K, M), rnd(g, phys if row.entry == 'tn_rows' else K, N, scale=s)
    case = dict(A=A, B=B, b1=rnd(g, N, scale=0.3), b2=rnd(g, N, scale=0.3), C0=rnd(g, phys if row.entry == 'nt_rows' else M, N), map=rmap, phys=phys)
    if row.act == ACT_MASK:
        assert M == len(row.lens) * row.T
        case.update(mul=rnd(g, M, N), mask0=rnd(g, M, N), lens=torch.tensor(row.lens))
    if row.M > 4096 and row.op == 'nt' and row.entry == 'gemm':
        case['A'][4096:] = case['A'][4096:] * 0.5 + 0.25          # the two sides of a row-tail boundary carry different values
    return case


def _act(v, act):
    if act == ACT_TANH:
        return torch.tanh(v)
    if act == ACT_RELU:
        return torch.clamp(v, min=0)
    if act == ACT_LRELU:
        return torch.where(v > 0, v, 0.2 * v)
    if act in (ACT_SIGMOID, ACT_MASK):
        return torch.sigmoid(v)
    assert act == ACT_NONE
    return v


def dense_ref(row, case, dtype=torch.float64, mistake=None, order='mm', rows=None, plan=None):
    """What the row's entry point leaves behind -> dict(C: (physical rows, N), mask_out: (M, N) for the mask epilogue, scale: the largest
    |op(A) op(B)|, the unit every error of the dense tests is measured in).  rows (a list of logical output rows): only those rows of C (and
    mask_out), in that order, nothing scattered.  float64: torch's product.  float32: the written-out orders -- 'mm' (refs64_conv._mm) or 'k2'
    (_mm_k2 over k_slices(row, plan)).  plan: the plan the product runs with (default: the one the row declares); only 'k2' and mistake 'd' read it."""
    plan = plan if plan is not None else row.plan
    A, B = case['A'].to(dtype), case['B'].to(dtype)
    if mistake == 'j':
        A, B = round11(A), round11(B)
    if mistake == 'k':
        A, B = round16(A), round16(B)
    M, N, K = row.M, row.N, row.K
    m = case['map']
    sel = torch.arange(M) if rows is None else torch.as_tensor(rows, dtype=torch.long)
    if m is not None and mistake == 'h':
        m = m.clone()
        j = int(sel[len(sel) // 2]) if row.entry == 'nt_rows' else len(m) // 2          # an output row that is looked at; a row of the contraction
        m[j] += 1 if int(m[j]) + 1 < case['phys'] else -1
    if row.op == 'nt':
        a, b = (A[m[sel]] if row.entry == 'nt_rows' else A[sel]), B.t()
    elif row.op == 'nn':
        a, b = A[sel], B
    else:
        a, b = (A[m] if row.entry == 'tn_rows' else A)[:, sel].t(), (B[m] if row.entry == 'tn_rows' else B)
    a, b = a.contiguous(), b.contiguous()
    if dtype == torch.float32:
        assert mistake is None
        prod = _mm(a, b) if order == 'mm' else _mm_k2(a, b, k_slices(row, plan))
    else:
        prod = a @ b
    scale = prod.abs().max().item()
    if mistake == 'a':
        prod = prod - a[:, K - 1, None] * b[None, K - 1, :]
    if mistake == 'd':
        if plan['route'] == 'pipeline':          # a 16-k unit of the last tile: the tail's tiles are the last ones
            bm, bn = (int(v) for v in plan['tile'].split('x')[:2])
            rs = torch.nonzero(sel >= (M - 1) // bm * bm).flatten()
            c0, k0, k1 = (N - 1) // bn * bn, 16, min(K, 32)
            prod[rs[:, None], torch.arange(c0, N)[None, :]] -= a[rs, k0:k1] @ b[k0:k1, c0:]
        else:
            sl = k_slices(row, plan)
            k0, k1 = sl[len(sl) // 2]
            prod = prod - a[:, k0:k1] @ b[k0:k1]
    pre = prod
    if row.bias:
        pre = pre + case['b1'].to(dtype)
    if row.bias2 and mistake != 'e':
        pre = pre + case['b2'].to(dtype)
    c0 = case['C0'].to(dtype)
    c0l = c0[m[sel]] if row.entry == 'nt_rows' else c0[sel]          # the prior content of the logical rows
    out = {}
    if row.act == ACT_MASK:
        t, bi = sel % row.T, sel // row.T
        live = (t <= case['lens'][bi]) if mistake == 'i' else (t < case['lens'][bi])
        mask = torch.where(live[:, None], torch.sigmoid(pre), torch.zeros_like(pre))
        val = mask * case['mul'].to(dtype)[sel]
        out['mask_out'] = mask
    elif row.beta and mistake == 'g':
        val = _act(pre + c0l, row.act)
    else:
        val = _act(pre, row.act)
        if row.beta and mistake != 'f':
            val = val + c0l
    if mistake == 'b' and len(sel) > 1:
        assert int(sel[-1]) == M - 1 and int(sel[-2]) == M - 2
        for t in [val] + list(out.values()):
            t[-1] = t[-2]
    if mistake == 'c':
        val[:, max(0, N - 4):] = c0l[:, max(0, N - 4):]
        if 'mask_out' in out:
            out['mask_out'][:, max(0, N - 4):] = case['mask0'].to(dtype)[sel][:, max(0, N - 4):]
    if rows is None and row.entry == 'nt_rows':
        C = c0.clone()
        C[m] = val
        val = C
    out.update(C=val, scale=scale)
    return out


def dense_err(got, ref):
    """max |got - ref| over C (and mask_out) in units of ref['scale']; inf where got is not finite."""
    worst = 0.0
    for k in ('C', 'mask_out'):
        if k in ref:
            d = (got[k].detach().double().cpu() - ref[k].double()).abs().max().item()
            worst = max(worst, d if math.isfinite(d) else float('inf'))
    return worst / ref['scale']


def mistakes_of(row, plan):
    """The MISTAKES that apply to a row under a plan."""
    m = ['a', 'c', 'j', 'k']
    if row.M > 1 and (row.act != ACT_MASK or row.lens[-1] >= row.T >= 2):          # (a mask row: the last two frames are live)
        m.append('b')
    if (plan['route'] == 'engine' and int(plan['splits']) > 1) or (plan['route'] == 'pipeline' and int(plan['g_sk']) > 0 and row.K > 16) or \
            (family_of(row, plan)[0] == 'skinny_wg' and row.K > 8):
        m.append('d')
    if row.bias2:
        m.append('e')
    if row.beta:
        m.append('f')
        if row.act != ACT_NONE:
            m.append('g')
    if row.rmap is not None:
        m.append('h')
    if row.act == ACT_MASK and any(l < row.T for l in row.lens):
        m.append('i')
    return sorted(m)


YARD_ROWS_ALL = 1 << 27          # products of up to this many multiply-adds are measured on every output row


def yard_rows(row):
    """The output rows the fp32 yardstick and the sensitivities of a large row are evaluated on (None: all): the first and the last row of every
    block of 64 rows -- every tile of the engine and of the pipeline is a whole number of such blocks, and so is a row-tail boundary m1 -- and the
    last two rows.  The GPU comparison always covers the whole matrix."""
    if row.M * row.N * row.K <= YARD_ROWS_ALL:
        return None
    return sorted({r for r in range(row.M) if r % 64 in (0, 63)} | {row.M - 2, row.M - 1})


def case_id(row):
    tag = 'edge' if row.form is None else '-'.join(str(v) for v in row.form)
    s = '%s-%s-%dx%dx%d-act%d' % (tag, row.op, row.M, row.N, row.K, row.act)
    s += ('-b%d%d' % (row.bias, row.bias2) if row.bias or row.bias2 else '') + ('-beta' if row.beta else '') + '-p%d.%d.%d' % row.pad
    s += ('-o%d%d%d' % row.off if any(row.off) else '') + ('-filler' if row.filler else '') + ('-' + row.entry if row.entry != 'gemm' else '')
    s += ('-n1.%d' % row.n1 if row.n1 else '') + ('-map%d.%d.%d.%d' % tuple(int(v) for v in row.rmap) if row.rmap else '') + ('-T%d-%s' % (row.T, '.'.join(str(l) for l in row.lens)) if row.lens else '')
    return s


# ---------------------------------------------------------------------------------------------
# the case table: one row per form re2e_gemm_plan can name on a 256-CU chip (tests/test_refs64_gemm_cpu.py: closed under a sweep of the plans),
# each at the smallest ragged shape that names it -- most below 64 x 72 x 523; the 256x128 tile from 2048 rows; a row tail from more than 256 tiles
# of 256x128; a pipeline schedule with whole tiles and a tail from more than 256 tiles; the all-tail schedule of variant 6 only where the 128x64
# tiles of variant 8 would NOT be all tail (more than 256 of them) and the product is long enough for the rates to decide (257 x 5504 x 3584).
# Epilogues differ from row to row (bias and bias2, the five activations, beta = 1); ldc > N everywhere (canary columns).  Rows on a FILLER
# stream: an engine row, a pipeline row, a mapped weight gradient.  The two forms below the plan come last.
# ---------------------------------------------------------------------------------------------
SKINNY2_PLAN = dict(route='skinny2')          # re2e_gemm_skinny2 has no plan: what family_of / k_slices / mistakes_of take in its place
LENS7 = (1, 293, 150, 292, 2, 77, 293)
DENSE_CASES = [
    _row(('skinny_wg', 'nt', 1), 'nt', 17, 33, 72, bias2=1, beta=1, plan=dict(route='skinny_wg', vec='1')),
    _row(('skinny_wg', 'nt', 0), 'nt', 32, 20, 66, pad=(3, 5, 3), plan=dict(route='skinny_wg', vec='0')),
    _row(('skinny_wg', 'nn', 1), 'nn', 31, 36, 100, bias2=1, plan=dict(route='skinny_wg', vec='1')),
    _row(('skinny_wg', 'nn', 0), 'nn', 5, 33, 65, beta=1, pad=(0, 3, 1), plan=dict(route='skinny_wg', vec='0')),
    _row(('engine', 'nn', 0, '128x128x16', 'one', 0, 0, 0), 'nn', 37, 70, 21, act=ACT_RELU, pad=(3, 2, 3), plan=dict(route='engine', vec='0', tile='128x128x16', splits='1', m1='37')),
    _row(('engine', 'nn', 1, '128x128x16', 'one', 0, 0, 0), 'nn', 37, 68, 20, act=ACT_LRELU, bias2=1, plan=dict(route='engine', vec='1', tile='128x128x16', splits='1', m1='37')),
    _row(('engine', 'nn', 0, '128x128x16', 'split', 0, 0, 0), 'nn', 45, 70, 522, act=ACT_TANH, pad=(3, 2, 3), plan=dict(route='engine', vec='0', tile='128x128x16', splits='2', m1='45')),
    _row(('engine', 'nn', 1, '128x128x16', 'split', 0, 0, 0), 'nn', 45, 68, 520, act=ACT_RELU, beta=1, plan=dict(route='engine', vec='1', tile='128x128x16', splits='2', m1='45')),
    _row(('engine', 'nn', 0, '128x128x16', 'zx', 0, 0, 0), 'nn', 45, 70, 2058, beta=1, pad=(3, 2, 3), plan=dict(route='engine', vec='0', tile='128x128x16', splits='8', m1='45')),
    _row(('engine', 'nn', 1, '128x128x16', 'zx', 0, 0, 0), 'nn', 45, 68, 2056, act=ACT_RELU, bias2=1, plan=dict(route='engine', vec='1', tile='128x128x16', splits='8', m1='45')),
    _row(('engine', 'nn', 0, '32x128x32', 'split', 0, 0, 0), 'nn', 8, 70, 202, act=ACT_TANH, bias2=1, pad=(3, 2, 3), plan=dict(route='engine', vec='0', tile='32x128x32', splits='3', m1='8')),
    _row(('engine', 'nn', 1, '32x128x32', 'split', 0, 0, 0), 'nn', 31, 68, 200, act=ACT_LRELU, beta=1, plan=dict(route='engine', vec='1', tile='32x128x32', splits='3', m1='31')),
    _row(('engine', 'nn', 0, '32x128x32', 'zx', 0, 0, 0), 'nn', 8, 70, 522, act=ACT_RELU, pad=(3, 2, 3), plan=dict(route='engine', vec='0', tile='32x128x32', splits='8', m1='8')),
    _row(('engine', 'nn', 1, '32x128x32', 'zx', 0, 0, 0), 'nn', 31, 68, 520, act=ACT_TANH, bias2=1, beta=1, plan=dict(route='engine', vec='1', tile='32x128x32', splits='8', m1='31')),
    _row(('engine', 'nt', 0, '128x128x16', 'one', 0, 0, 0), 'nt', 37, 70, 21, act=ACT_TANH, pad=(3, 2, 3), plan=dict(route='engine', vec='0', tile='128x128x16', splits='1', m1='37')),
    _row(('engine', 'nt', 1, '128x128x16', 'one', 0, 0, 0), 'nt', 37, 70, 20, act=ACT_RELU, bias2=1, beta=1, plan=dict(route='engine', vec='1', tile='128x128x16', splits='1', m1='37')),
    _row(('engine', 'nt', 0, '128x128x16', 'one', 0, 1, 0), 'nt', 39, 70, 21, act=ACT_MASK, pad=(3, 2, 3), T=13, lens=(1, 7, 13), plan=dict(route='engine', vec='0', tile='128x128x16', splits='1', m1='39')),
    _row(('engine', 'nt', 1, '128x128x16', 'one', 0, 1, 0), 'nt', 39, 68, 20, act=ACT_MASK, bias2=1, T=13, lens=(5, 13, 12), plan=dict(route='engine', vec='1', tile='128x128x16', splits='1', m1='39')),
    _row(('engine', 'nt', 0, '128x128x16', 'split', 0, 0, 0), 'nt', 45, 70, 522, act=ACT_LRELU, pad=(3, 2, 3), plan=dict(route='engine', vec='0', tile='128x128x16', splits='2', m1='45')),
    _row(('engine', 'nt', 1, '128x128x16', 'split', 0, 0, 0), 'nt', 45, 70, 520, act=ACT_SIGMOID, bias2=1, plan=dict(route='engine', vec='1', tile='128x128x16', splits='2', m1='45')),
    _row(('engine', 'nt', 0, '128x128x16', 'zx', 0, 0, 0), 'nt', 45, 70, 2058, bias2=1, pad=(3, 2, 3), plan=dict(route='engine', vec='0', tile='128x128x16', splits='8', m1='45')),
    _row(('engine', 'nt', 1, '128x128x16', 'zx', 0, 0, 0), 'nt', 45, 70, 2056, act=ACT_TANH, beta=1, plan=dict(route='engine', vec='1', tile='128x128x16', splits='8', m1='45')),
    _row(('engine', 'nt', 0, '32x128x32', 'one', 0, 1, 0), 'nt', 30, 70, 131, act=ACT_MASK, pad=(3, 2, 3), T=10, lens=(4, 1, 10), plan=dict(route='engine', vec='0', tile='32x128x32', splits='1', m1='30')),
    _row(('engine', 'nt', 1, '32x128x32', 'one', 0, 1, 0), 'nt', 30, 68, 132, act=ACT_MASK, T=6, lens=(6, 6, 3, 1, 5), plan=dict(route='engine', vec='1', tile='32x128x32', splits='1', m1='30')),
    _row(('engine', 'nt', 0, '32x128x32', 'split', 0, 0, 0), 'nt', 8, 70, 202, act=ACT_RELU, beta=1, pad=(3, 2, 3), plan=dict(route='engine', vec='0', tile='32x128x32', splits='3', m1='8')),
    _row(('engine', 'nt', 1, '32x128x32', 'split', 0, 0, 0), 'nt', 31, 68, 200, act=ACT_TANH, bias2=1, plan=dict(route='engine', vec='1', tile='32x128x32', splits='3', m1='31')),
    _row(('engine', 'nt', 0, '32x128x32', 'zx', 0, 0, 0), 'nt', 8, 70, 522, act=ACT_LRELU, pad=(3, 2, 3), plan=dict(route='engine', vec='0', tile='32x128x32', splits='8', m1='8')),
    _row(('engine', 'nt', 1, '32x128x32', 'zx', 0, 0, 0), 'nt', 31, 68, 8196, beta=1, plan=dict(route='engine', vec='1', tile='32x128x32', splits='64', m1='31')),
    _row(('engine', 'nt', 1, '256x128x16', 'one', 0, 0, 0), 'nt', 2051, 70, 20, act=ACT_LRELU, bias2=1, plan=dict(route='engine', vec='1', tile='256x128x16', splits='1', m1='2051')),
    _row(('engine', 'nt', 1, '256x128x16', 'one', 0, 1, 0), 'nt', 2051, 68, 20, act=ACT_MASK, pad=(4, 8, 2), T=293, lens=LENS7, plan=dict(route='engine', vec='1', tile='256x128x16', splits='1', m1='2051')),
    _row(('engine', 'nt', 1, '256x128x16', 'one', 1, 0, 0), 'nt', 4352, 2046, 20, act=ACT_RELU, plan=dict(route='engine', vec='1', tile='256x128x16', splits='1', m1='4096')),
    _row(('engine', 'nt', 1, '256x128x16', 'split', 0, 0, 0), 'nt', 2051, 70, 520, act=ACT_TANH, bias2=1, plan=dict(route='engine', vec='1', tile='256x128x16', splits='2', m1='2051')),
    _row(('engine', 'nt', 1, '256x128x16', 'zx', 0, 0, 0), 'nt', 2051, 70, 2056, act=ACT_LRELU, beta=1, plan=dict(route='engine', vec='1', tile='256x128x16', splits='8', m1='2051')),
    _row(('engine', 'nt', 1, '128x128x16', 'one', 0, 0, 0), 'nt', 2051, 70, 20, filler=True, plan=dict(route='engine', vec='1', tile='128x128x16', splits='1', m1='2051')),
    _row(('engine', 'tn', 0, '128x128x16', 'one', 0, 0, 0), 'tn', 37, 70, 21, beta=1, pad=(3, 2, 3), plan=dict(route='engine', vec='0', tile='128x128x16', splits='1', m1='37')),
    _row(('engine', 'tn', 0, '128x128x16', 'split', 0, 0, 0), 'tn', 37, 70, 523, pad=(3, 2, 3), plan=dict(route='engine', vec='0', tile='128x128x16', splits='2', m1='37')),
    _row(('engine', 'tn', 0, '128x128x16', 'zx', 0, 0, 0), 'tn', 37, 70, 2059, act=ACT_RELU, pad=(3, 2, 3), plan=dict(route='engine', vec='0', tile='128x128x16', splits='8', m1='37')),
    _row(('engine', 'tn', 1, '128x128x16', 'one', 0, 0, 0), 'tn', 36, 68, 21, plan=dict(route='engine', vec='1', tile='128x128x16', splits='1', m1='36')),
    _row(('engine', 'tn', 1, '128x128x16', 'split', 0, 0, 0), 'tn', 36, 68, 523, beta=1, plan=dict(route='engine', vec='1', tile='128x128x16', splits='2', m1='36')),
    _row(('engine', 'tn', 1, '128x128x16', 'zx', 0, 0, 0), 'tn', 36, 68, 2059, plan=dict(route='engine', vec='1', tile='128x128x16', splits='8', m1='36')),
    _row(('engine', 'tn', 1, '256x128x16', 'one', 0, 0, 0), 'tn', 2048, 68, 21, beta=1, plan=dict(route='engine', vec='1', tile='256x128x16', splits='1', m1='2048')),
    _row(('engine', 'tn', 1, '256x128x16', 'split', 0, 0, 0), 'tn', 2048, 68, 523, plan=dict(route='engine', vec='1', tile='256x128x16', splits='2', m1='2048')),
    _row(('engine', 'tn', 1, '256x128x16', 'zx', 0, 0, 0), 'tn', 2048, 68, 2059, beta=1, plan=dict(route='engine', vec='1', tile='256x128x16', splits='8', m1='2048')),
    _row(('engine', 'tn', 1, '128x128x16', 'one', 0, 0, 1), 'tn', 36, 68, 70, entry='tn_rows', rmap=(20, 16, 0, 3), plan=dict(route='engine', vec='1', tile='128x128x16', splits='1', m1='36')),
    _row(('engine', 'tn', 1, '128x128x16', 'split', 0, 0, 1), 'tn', 36, 68, 523, beta=1, entry='tn_rows', rmap=(100, 100, 0, 0), plan=dict(route='engine', vec='1', tile='128x128x16', splits='2', m1='36')),
    _row(('engine', 'tn', 1, '128x128x16', 'zx', 0, 0, 1), 'tn', 36, 68, 2059, entry='tn_rows', rmap=(0, 0, 1, 2), plan=dict(route='engine', vec='1', tile='128x128x16', splits='8', m1='36')),
    _row(('engine', 'tn', 1, '128x128x16', 'zx', 0, 0, 1), 'tn', 2048, 68, 2059, beta=1, filler=True, entry='tn_rows', rmap=(1000, 512, 0, 1), plan=dict(route='engine', vec='1', tile='128x128x16', splits='8', m1='2048')),
    _row(('engine', 'tn', 1, '256x128x16', 'one', 0, 0, 1), 'tn', 2048, 68, 70, beta=1, entry='tn_rows', rmap=(16, 16, 0, 3), plan=dict(route='engine', vec='1', tile='256x128x16', splits='1', m1='2048')),
    _row(('engine', 'tn', 1, '256x128x16', 'split', 0, 0, 1), 'tn', 2048, 68, 523, entry='tn_rows', rmap=(40, 33, 0, 0), plan=dict(route='engine', vec='1', tile='256x128x16', splits='2', m1='2048')),
    _row(('engine', 'tn', 1, '256x128x16', 'zx', 0, 0, 1), 'tn', 2048, 68, 2059, entry='tn_rows', rmap=(2059, 2059, 0, 5), plan=dict(route='engine', vec='1', tile='256x128x16', splits='8', m1='2048')),
    _row(('pipeline', 3, 'dp', 0), 'nt', 2305, 1668, 20, act=ACT_TANH, bias2=1, plan=dict(route='pipeline', variant='3', tile='256x128x16', n_dp='140', g_sk='0')),
    _row(('pipeline', 3, 'dp+sk', 0), 'nt', 6400, 2048, 260, act=ACT_RELU, bias2=1, beta=1, plan=dict(route='pipeline', variant='3', tile='256x128x16', n_dp='256', g_sk='256')),
    _row(('pipeline', 6, 'dp', 0), 'nt', 7777, 260, 36, act=ACT_LRELU, plan=dict(route='pipeline', variant='6', tile='128x128x16', n_dp='183', g_sk='0')),
    _row(('pipeline', 6, 'dp', 1), 'nt', 7777, 260, 36, act=ACT_SIGMOID, bias2=1, entry='nt_rows', rmap=(4000, 128, 0, 0), plan=dict(route='pipeline', variant='6', tile='128x128x16', n_dp='183', g_sk='0')),
    _row(('pipeline', 6, 'dp+sk', 0), 'nt', 6400, 1024, 260, act=ACT_TANH, beta=1, filler=True, plan=dict(route='pipeline', variant='6', tile='128x128x16', n_dp='256', g_sk='256')),
    _row(('pipeline', 6, 'dp+sk', 1), 'nt', 3073, 2048, 260, act=ACT_RELU, entry='nt_rows', rmap=(1000, 1000, 0, 2), plan=dict(route='pipeline', variant='6', tile='128x128x16', n_dp='256', g_sk='256')),
    _row(('pipeline', 8, 'dp', 0), 'nt', 300, 68, 36, bias2=1, beta=1, plan=dict(route='pipeline', variant='8', tile='128x64x16', n_dp='6', g_sk='0')),
    _row(('pipeline', 8, 'dp', 1), 'nt', 300, 68, 36, act=ACT_TANH, entry='nt_rows', rmap=(0, 0, 1, 0), plan=dict(route='pipeline', variant='8', tile='128x64x16', n_dp='6', g_sk='0')),
    _row(('pipeline', 8, 'dp+sk', 0), 'nt', 12800, 132, 516, act=ACT_RELU, bias2=1, plan=dict(route='pipeline', variant='8', tile='128x64x16', n_dp='256', g_sk='176')),
    _row(('pipeline', 8, 'dp+sk', 1), 'nt', 7777, 260, 516, act=ACT_LRELU, beta=1, entry='nt_rows', rmap=(128, 100, 0, 1), plan=dict(route='pipeline', variant='8', tile='128x64x16', n_dp='256', g_sk='200')),
    _row(('pipeline', 8, 'sk', 0), 'nt', 300, 68, 516, act=ACT_RELU, beta=1, plan=dict(route='pipeline', variant='8', tile='128x64x16', n_dp='0', g_sk='24')),
    _row(('pipeline', 8, 'sk', 1), 'nt', 300, 68, 516, bias2=1, entry='nt_rows', rmap=(129, 129, 0, 0), plan=dict(route='pipeline', variant='8', tile='128x64x16', n_dp='0', g_sk='24')),
    _row(('pipeline', 6, 'sk', 0), 'nt', 257, 5504, 3584, act=ACT_TANH, bias2=1, plan=dict(route='pipeline', variant='6', tile='128x128x16', n_dp='0', g_sk='256')),
    _row(('pipeline', 6, 'sk', 1), 'nt', 257, 5504, 3584, beta=1, entry='nt_rows', rmap=(200, 64, 0, 1), plan=dict(route='pipeline', variant='6', tile='128x128x16', n_dp='0', g_sk='256')),
    # the mask epilogue on x W and x^T W: re2e_gemm takes it in every operand form (a run-time branch of every engine instantiation; row = b T + t
    # of the OUTPUT), ops.py asks for it on x W^T alone
    _row(('engine', 'nn', 0, '128x128x16', 'one', 0, 1, 0), 'nn', 39, 70, 21, act=ACT_MASK, pad=(3, 2, 3), T=13, lens=(1, 7, 13), plan=dict(route='engine', vec='0', tile='128x128x16', splits='1', m1='39')),
    _row(('engine', 'nn', 1, '128x128x16', 'one', 0, 1, 0), 'nn', 39, 68, 20, act=ACT_MASK, bias2=1, T=13, lens=(5, 12, 13), plan=dict(route='engine', vec='1', tile='128x128x16', splits='1', m1='39')),
    _row(('engine', 'nn', 0, '32x128x32', 'one', 0, 1, 0), 'nn', 30, 70, 131, act=ACT_MASK, pad=(3, 2, 3), T=10, lens=(4, 1, 10), plan=dict(route='engine', vec='0', tile='32x128x32', splits='1', m1='30')),
    _row(('engine', 'nn', 1, '32x128x32', 'one', 0, 1, 0), 'nn', 30, 68, 132, act=ACT_MASK, bias2=1, T=6, lens=(6, 5, 3, 1, 6), plan=dict(route='engine', vec='1', tile='32x128x32', splits='1', m1='30')),
    _row(('engine', 'tn', 0, '128x128x16', 'one', 0, 1, 0), 'tn', 39, 70, 21, act=ACT_MASK, pad=(3, 2, 3), T=13, lens=(1, 7, 13), plan=dict(route='engine', vec='0', tile='128x128x16', splits='1', m1='39')),
    _row(('engine', 'tn', 1, '128x128x16', 'one', 0, 1, 0), 'tn', 36, 68, 21, act=ACT_MASK, bias2=1, T=12, lens=(5, 11, 12), plan=dict(route='engine', vec='1', tile='128x128x16', splits='1', m1='36')),
    _row(('engine', 'tn', 1, '256x128x16', 'one', 0, 1, 0), 'tn', 2048, 68, 21, act=ACT_MASK, T=256, lens=(1, 256, 150, 255, 2, 77, 3, 256), plan=dict(route='engine', vec='1', tile='256x128x16', splits='1', m1='2048')),
    # the 32x128 tile with ONE slice and no mask: pick_splits_skinny wants ceil(192 / column tiles) slices, so only from 192 column tiles (N > 24 448)
    _row(('engine', 'nt', 0, '32x128x32', 'one', 0, 0, 0), 'nt', 8, 24578, 131, act=ACT_TANH, pad=(3, 2, 3), plan=dict(route='engine', vec='0', tile='32x128x32', splits='1', m1='8')),
    _row(('engine', 'nt', 1, '32x128x32', 'one', 0, 0, 0), 'nt', 8, 24578, 132, act=ACT_RELU, bias2=1, beta=1, plan=dict(route='engine', vec='1', tile='32x128x32', splits='1', m1='8')),
    _row(('engine', 'nn', 0, '32x128x32', 'one', 0, 0, 0), 'nn', 8, 24578, 131, act=ACT_LRELU, pad=(3, 2, 3), beta=1, plan=dict(route='engine', vec='0', tile='32x128x32', splits='1', m1='8')),
    _row(('engine', 'nn', 1, '32x128x32', 'one', 0, 0, 0), 'nn', 8, 24580, 132, act=ACT_LRELU, bias2=1, plan=dict(route='engine', vec='1', tile='32x128x32', splits='1', m1='8')),
    # the run-time fallback: a shape whose plan is the pipeline with a stream-K tail (variant 8, 256 whole tiles + 200 workgroups of tail), called with
    # a NULL workspace, runs the engine's plan for it -- which has to be one without a split (a split engine plan without workspace is an error:
    # tests/test_dense_kernels_gpu.py::test_mapped_entry_points_refuse_what_they_do_not_run)
    _row(('below_plan', 'fallback', 'engine', 'nt', 1, '256x128x16', 'one', 0, 0, 0), 'nt', 7777, 260, 516, act=ACT_TANH, bias2=1, entry='gemm_nows', plan=dict(route='engine', vec='1', tile='256x128x16', splits='1', m1='7777')),
    _row(('below_plan', 'skinny2'), 'nn', 17, 61, 100, pad=(4, 3, 1), entry='skinny2', n1=33, plan=SKINNY2_PLAN),
]

# Built and never named by a plan on any shape of the sweep (kept out of the closure, with the reason): input for a later clean-up.
NEVER_NAMED = {
    ('pipeline', 3, 'sk', 0): 'the all-tail schedule of the 256x128 variant: no shape of the sweep, nor of a search over every tile count below 256 with K up '
                              'to 12 800, names it -- where fewer than 256 tiles of 256x128 are the whole product the cost model (nt2_plan_variant) '
                              'prices the hand-off of 128 KiB slabs above the 128x64 variant\'s, which cuts the same product into four times as many tiles',
    ('pipeline', 3, 'dp', 1): 'variant 3 through a row map: nt2_plan is asked for 4-wave tiles only for every mapped product (in.filler || in.rowmap)',
    ('pipeline', 3, 'dp+sk', 1): 'the same with a stream-K tail',
    ('pipeline', 3, 'sk', 1): 'the same, all tail',
}


# ---------------------------------------------------------------------------------------------
# Edges.  form None: an edge names no form of its own, but it DECLARES the kernel family it is there to turn -- route, then the pipeline's variant
# or the engine's tile and whether K is split -- and both test files assert it (plan_matches), so an edge cannot drift onto another kernel either.
# ---------------------------------------------------------------------------------------------
def _want(text):
    """'pipeline 8' / 'engine 128x128x16' / 'engine 128x128x16 split' / 'skinny_wg' -> the partial plan an edge declares ('split': splits > 1)."""
    w = text.split()
    if w[0] == 'pipeline':
        return dict(route=w[0], variant=w[1])
    if w[0] == 'engine':
        return dict(route=w[0], tile=w[1], split=str(int(len(w) > 2)))
    return dict(route=w[0])


def plan_matches(declared, plan):
    """Every entry of a declared (partial) plan is what a re2e_gemm_plan answer holds."""
    return all((int(plan.get('splits', 1)) > 1) == (v == '1') if k == 'split' else plan.get(k) == v for k, v in declared.items())


def _edges():
    e = []

    def E(want, op, M, N, K, **kw):
        e.append(_row(None, op, M, N, K, plan=_want(want), **kw))

    # ---- pipeline, per variant, each shape on the variant it declares (found by a search over tile counts: the cost model moves between the
    # variants with the tile count, so the edges of one variant sit at different sizes): M one below / at / above a tile row and 2 bm + 3; N four
    # below / at / four above a tile column; K of 4, 12, 16, 20, 36 and 16 k + 4 (N and K stay multiples of 4, or the pipeline declines).
    # variant 8 (128x64); M = 255 is the engine's side of the pipeline's floor of 256 rows
    E('engine 128x128x16', 'nt', 255, 68, 36, act=ACT_TANH, bias2=1)
    for M in (256, 257, 259, 383, 384, 385):
        E('pipeline 8', 'nt', M, 68, 36, act=ACT_TANH, bias2=1)
    for N in (60, 64, 68):
        E('pipeline 8', 'nt', 300, N, 36, act=ACT_RELU, beta=1)
    for K in (4, 12, 16, 20, 84):
        E('pipeline 8', 'nt', 300, 68, K, act=ACT_SIGMOID)
    for M, N, K in ((7777, 252, 36), (7777, 256, 36), (2305, 1668, 36), (2305, 1668, 84)):          # the same N and K edges at many rows
        E('pipeline 8', 'nt', M, N, K, act=ACT_LRELU, bias2=1)
    # variant 6 (128x128): M = 52 bm - 1, 52 bm, 60 bm - 1, 60 bm, 60 bm + 1, 3 bm + 1, 2 bm + 3; N = 33 bn - 4, 33 bn, 32 bn + 4, 13 bn - 4, 13 bn; K
    for M, N, K in ((6655, 260, 20), (6656, 260, 20), (7679, 260, 36), (7680, 260, 36), (7681, 260, 36), (259, 5508, 20), (385, 4220, 20), (385, 4224, 20),
                    (2303, 1668, 20), (2304, 1668, 20), (2305, 1660, 20), (2305, 1664, 20)) + \
            tuple((385, 4100, K) for K in (4, 12, 16, 20, 36, 84)) + tuple((7777, 260, K) for K in (4, 12, 16, 20, 84)):
        E('pipeline 6', 'nt', M, N, K, act=ACT_LRELU, bias2=1)
    # variant 3 (256x128, 8 waves): M = 52 bm - 1, 52 bm, 51 bm + 1, 10 bm + 3, 2 bm + 3; N = 29 bn - 4, 29 bn, 2 bn + 4, 13 bn + 4; K (36 and 84 only
    # from 56 x 4 tiles: below, the 128x64 variant is cheaper at those K)
    for M, N, K in ((13311, 260, 20), (13312, 260, 20), (13057, 260, 20), (2563, 1668, 20), (515, 6532, 20), (1025, 3708, 20), (1025, 3712, 20),
                    (13057, 260, 4), (13057, 260, 12), (13057, 260, 16), (2305, 1668, 4), (2305, 1668, 12), (2305, 1668, 16), (14081, 388, 36), (14081, 388, 84)):
        E('pipeline 3', 'nt', M, N, K, act=ACT_TANH, beta=1)
    # the stream-K tail's cuts on 6 tiles of 128x64 (300 x 68): K = 132 and 260 stay whole tiles (the model does not cut 9 or 17 k-tiles), 1028
    # (65 k-tiles) is cut for 48 workgroups of 8.125 units: every boundary inside a tile, 9 parts per tile (parts > 3 in nt2_plan_variant; the
    # table's 300 x 68 x 516 row has 5).  At most three parts per cut tile: 1000 x 1028 x 676, 136 tiles of 43 k-tiles on 256 workgroups of 22.8 units
    for K in (132, 260, 1028):
        E('pipeline 8', 'nt', 300, 68, K, bias2=1, beta=1)
    E('pipeline 8', 'nt', 1000, 1028, 676, act=ACT_TANH, bias2=1, beta=1)
    # ---- engine: the three axes around the 128x128 tile without 16-byte loads (N % 4 != 0 drops them in x W, K % 4 != 0 in x W^T) and with them
    for op in ('nt', 'nn', 'tn'):
        for M, N, K in ((127, 70, 21), (128, 70, 21), (129, 70, 21), (259, 70, 21), (37, 127, 21), (37, 129, 21), (37, 70, 15), (37, 70, 17), (37, 70, 33),
                        (124, 68, 20), (128, 128, 16), (132, 132, 36), (36, 124, 12), (36, 132, 4), (36, 68, 84)):
            E('engine 128x128x16', op, M, N, K, act=ACT_RELU if op != 'tn' else ACT_NONE, bias2=int(op == 'tn'), beta=int(K % 2 == 0), pad=(3, 2, 3) if K % 4 else (4, 8, 4))
        # K no multiple of 16 x splits, a last slice shorter than the others
        E('engine 128x128x16 split', op, 45, 70, 1000, pad=(3, 2, 3))
        E('engine 128x128x16 split', op, 44, 68, 1000, beta=1)
        # a base pointer one float behind a 16-byte boundary: A, B, C in turn
        for off in ((1, 0, 0), (0, 1, 0), (0, 0, 1)):
            E('engine 128x128x16', op, 36, 68, 20, off=off, bias2=1)
            E('engine 128x128x16 split', op, 300, 68, 516, off=off)
    E('engine 128x128x16 split', 'tn', 38, 68, 523)          # M % 4 != 0 drops the 16-byte loads of x^T W
    E('engine 128x128x16 split', 'tn', 2050, 68, 523, beta=1)
    # the 32x128 tile (M <= 32 with an activation): M of 1, 31, 32; N around 128; K around its k-tile of 32
    for M, N, K in ((1, 68, 200), (32, 68, 200), (31, 127, 200), (31, 128, 200), (31, 129, 131), (31, 68, 129), (31, 68, 160), (8, 70, 161)):
        E('engine 32x128x32 split', 'nt', M, N, K, act=ACT_TANH, bias2=1)
        E('engine 32x128x32 split', 'nn', M, N, K, act=ACT_LRELU, beta=1, pad=(3, 2, 3) if N % 4 else (4, 8, 4))
    # the 256x128 tile: its floor of 2048 rows, a ragged second tile row; the row tail with beta = 1 and on a filler stream (no tail there)
    E('engine 128x128x16', 'nt', 2047, 70, 20, act=ACT_SIGMOID, beta=1)
    for M in (2048, 2049, 2307):
        E('engine 256x128x16', 'nt', M, 70, 20, act=ACT_SIGMOID, beta=1)
    E('engine 256x128x16', 'nt', 4352, 2046, 20, beta=1)
    E('engine 128x128x16', 'nt', 4352, 2046, 20, act=ACT_TANH, filler=True)
    # ---- skinny: every M, N and K of the kernel's edges with and without beta, both operand forms (K = 72: nine k-groups, three wavefronts idle;
    # 65: the scalar path; 8192: the longest contraction the route takes)
    for op in ('nt', 'nn'):
        for beta in (0, 1):
            for M, N, K in [(M, 33, 100) for M in (1, 31, 32)] + [(31, N, 72) for N in (1, 31, 32, 33)] + [(32, 33, K) for K in (64, 65, 68, 72, 100, 8192)]:
                E('skinny_wg', op, M, N, K, bias2=beta, beta=beta, pad=(4, 8, 4) if K % 4 == 0 and beta else (3, 1, 2))
    for M, N, n1, K, pad in ((1, 2, 1, 64, (4, 4, 4)), (32, 65, 32, 65, (3, 1, 2)), (32, 66, 33, 72, (4, 8, 4)), (31, 40, 9, 1200, (4, 0, 0)), (8, 64, 31, 8192, (0, 3, 5))):
        e.append(_row(None, 'nn', M, N, K, entry='skinny2', n1=n1, pad=pad, plan=SKINNY2_PLAN))
    # ---- row maps, x W^T: ident_rows of 0, inside the first tile, on a tile boundary, Mv; a descending map; the last entry the last physical row
    # or not; Mv = 256 exactly (the pipeline's floor)
    for rmap in ((50, 0, 0, 0), (50, 50, 0, 3), (128, 128, 0, 0), (300, 300, 0, 2), (0, 0, 1, 3), (200, 130, 0, 1)):
        E('pipeline 8', 'nt', 300, 68, 36, act=ACT_TANH, bias2=1, entry='nt_rows', rmap=rmap)
        E('pipeline 8', 'nt', 300, 68, 516, beta=1, entry='nt_rows', rmap=rmap)
    E('pipeline 8', 'nt', 256, 68, 36, act=ACT_RELU, entry='nt_rows', rmap=(100, 100, 0, 0))
    # x^T W: Kv = 64 (its floor), a Kv that leaves a partial k-tile; ident_rows of 0, inside the first k-tile, on a k-tile boundary, Kv; descending
    for K, rmap in ((64, (10, 0, 0, 0)), (64, (64, 64, 0, 3)), (70, (10, 10, 0, 0)), (70, (32, 32, 0, 1)), (70, (0, 0, 1, 0)), (523, (512, 512, 0, 0)), (523, (7, 7, 0, 2)),
                    (523, (0, 0, 1, 2)), (2059, (1030, 1024, 0, 0))):
        E('engine 128x128x16' + (' split' if K > 70 else ''), 'tn', 36, 68, K, beta=int(K == 70), entry='tn_rows', rmap=rmap)
    # ---- the mask epilogue: lengths of 1 and T, one in the middle, row counts that are no multiple of the tile; all utterances full; all of length 1
    E('engine 128x128x16', 'nt', 130, 68, 36, act=ACT_MASK, bias2=1, T=13, lens=(1, 13, 7, 13, 12, 2, 1, 9, 6, 13))
    E('engine 128x128x16', 'nt', 260, 70, 21, act=ACT_MASK, T=20, lens=(20,) * 13, pad=(3, 2, 3))
    E('engine 128x128x16', 'nt', 260, 68, 36, act=ACT_MASK, T=20, lens=(1,) * 13)
    E('engine 32x128x32', 'nt', 31, 68, 200, act=ACT_MASK, bias2=1, T=31, lens=(17,))
    E('engine 256x128x16', 'nt', 2307, 68, 20, act=ACT_MASK, T=769, lens=(1, 300, 769))
    E('engine 128x128x16', 'nn', 130, 70, 36, act=ACT_MASK, T=13, lens=(13, 1, 7, 13, 12, 2, 1, 9, 6, 13), pad=(4, 2, 3))
    E('engine 128x128x16', 'tn', 132, 68, 84, act=ACT_MASK, bias2=1, T=12, lens=(1, 12, 7, 12, 11, 2, 1, 9, 6, 3, 12))
    seen, out = set(), []
    for row in e:          # (32 x 33 x 100 is both an M edge and a K edge of the skinny kernels)
        if case_id(row) not in seen:
            seen.add(case_id(row))
            out.append(row)
    return out


EDGES = _edges()


# ---------------------------------------------------------------------------------------------
# The bars: 8 x the worst distance of the fp32 CPU yardstick from float64 over every row of DENSE_CASES and EDGES of the key, rounded up to one
# significant digit (tests/test_refs64_gemm_cpu.py recomputes the measured values and asserts every row within an eighth of its bar; no bar may
# exceed BAR_CAP, half the 2e-5 of the older dense tests).  The unit is the project's: max |got - float64| over the largest |op(A) op(B)| of
# the product; tanh and sigmoid have slope <= 1, so their outputs are held to the same bar.  Key: (family, K class) -> (bar, measured worst).
# YARDSTICK: the written-out fp32 order a family is measured with -- 'mm' (refs64_conv._mm: blocks of 32 terms summed pairwise, the blocks in
# sequence) for every family: on the MI355X every family stays inside 8 x that order (tests/test_dense_kernels_gpu.py prints both), so none had
# to move to the strictly sequential 'k2' order.
# ---------------------------------------------------------------------------------------------
BAR_CAP = 1e-5
YARDSTICK = {'skinny_wg': 'mm', 'pipeline': 'mm', 'engine': 'mm', 'engine_split': 'mm', 'mask': 'mm'}
BARS = {
    ('engine', 'K<=1024'): (2e-06, 1.705e-07),
    ('engine_split', 'K<=1024'): (3e-06, 2.663e-07),
    ('engine_split', 'K>1024'): (5e-06, 5.965e-07),
    ('mask', 'K<=1024'): (7e-07, 8.571e-08),
    ('pipeline', 'K<=1024'): (2e-06, 2.141e-07),
    ('pipeline', 'K>1024'): (4e-06, 4.261e-07),
    ('skinny_wg', 'K<=1024'): (2e-06, 1.804e-07),
    ('skinny_wg', 'K>1024'): (5e-06, 5.391e-07),
}

# Mistake (k) -- both operands rounded to 16 mantissa bits, what a two-term bf16 split carries -- moves every row but these by more than 1.5 bars
# on the CPU (tests/test_refs64_gemm_cpu.py asserts the split both ways, and more than 1 bar on the others): the rows listed here would not tell
# such a kernel from fp32.  DESIGN.md section 4.1 says which families they leave uncovered.
BLIND_TO_BF16X2 = (
    'engine-nn-0-128x128x16-split-0-0-0-nn-45x70x522-act1-b10-p3.2.3',          # 1.22 bars
    'engine-nn-1-128x128x16-split-0-0-0-nn-45x68x520-act2-b10-beta-p4.8.4',          # 1.32 bars
    'engine-nn-0-128x128x16-zx-0-0-0-nn-45x70x2058-act0-b10-beta-p3.2.3',          # 1.04 bars
    'engine-nn-1-128x128x16-zx-0-0-0-nn-45x68x2056-act2-b11-p4.8.4',          # 0.77 bars
    'engine-nn-0-32x128x32-split-0-0-0-nn-8x70x202-act1-b11-p3.2.3',          # 1.35 bars
    'engine-nn-1-32x128x32-split-0-0-0-nn-31x68x200-act3-b10-beta-p4.8.4',          # 1.26 bars
    'engine-nn-1-32x128x32-zx-0-0-0-nn-31x68x520-act1-b11-beta-p4.8.4',          # 1.40 bars
    'engine-nt-0-128x128x16-split-0-0-0-nt-45x70x522-act3-b10-p3.2.3',          # 1.42 bars
    'engine-nt-1-128x128x16-split-0-0-0-nt-45x70x520-act4-b11-p4.8.4',          # 0.33 bars
    'engine-nt-0-128x128x16-zx-0-0-0-nt-45x70x2058-act0-b11-p3.2.3',          # 0.92 bars
    'engine-nt-1-128x128x16-zx-0-0-0-nt-45x70x2056-act1-b10-beta-p4.8.4',          # 0.83 bars
    'engine-nt-0-32x128x32-split-0-0-0-nt-8x70x202-act2-b10-beta-p3.2.3',          # 1.08 bars
    'engine-nt-1-32x128x32-zx-0-0-0-nt-31x68x8196-act0-b10-beta-p4.8.4',          # 0.99 bars
    'engine-nt-1-256x128x16-split-0-0-0-nt-2051x70x520-act1-b11-p4.8.4',          # 1.42 bars
    'engine-nt-1-256x128x16-zx-0-0-0-nt-2051x70x2056-act3-b10-beta-p4.8.4',          # 0.97 bars
    'engine-tn-0-128x128x16-zx-0-0-0-tn-37x70x2059-act2-b10-p3.2.3',          # 0.85 bars
    'engine-tn-1-128x128x16-split-0-0-0-tn-36x68x523-act0-b10-beta-p4.8.4',          # 1.43 bars
    'engine-tn-1-128x128x16-zx-0-0-0-tn-36x68x2059-act0-b10-p4.8.4',          # 0.83 bars
    'engine-tn-1-256x128x16-split-0-0-0-tn-2048x68x523-act0-b10-p4.8.4',          # 1.41 bars
    'engine-tn-1-256x128x16-zx-0-0-0-tn-2048x68x2059-act0-b10-beta-p4.8.4',          # 0.87 bars
    'engine-tn-1-128x128x16-split-0-0-1-tn-36x68x523-act0-beta-p4.8.4-tn_rows-map100.100.0.0',          # 1.36 bars
    'engine-tn-1-128x128x16-zx-0-0-1-tn-36x68x2059-act0-p4.8.4-tn_rows-map0.0.1.2',          # 0.87 bars
    'engine-tn-1-128x128x16-zx-0-0-1-tn-2048x68x2059-act0-beta-p4.8.4-filler-tn_rows-map1000.512.0.1',          # 0.79 bars
    'engine-tn-1-256x128x16-zx-0-0-1-tn-2048x68x2059-act0-p4.8.4-tn_rows-map2059.2059.0.5',          # 1.08 bars
    'pipeline-6-dp-1-nt-7777x260x36-act4-b11-p4.8.4-nt_rows-map4000.128.0.0',          # 0.59 bars
    'pipeline-6-sk-0-nt-257x5504x3584-act1-b11-p4.8.4',          # 0.95 bars
    'pipeline-6-sk-1-nt-257x5504x3584-act0-b10-beta-p4.8.4-nt_rows-map200.64.0.1',          # 1.31 bars
    'edge-nt-300x68x4-act4-b10-p4.8.4',          # 0.57 bars
    'edge-nt-300x68x12-act4-b10-p4.8.4',          # 0.77 bars
    'edge-nt-300x68x16-act4-b10-p4.8.4',          # 0.71 bars
    'edge-nt-300x68x20-act4-b10-p4.8.4',          # 0.59 bars
    'edge-nt-300x68x84-act4-b10-p4.8.4',          # 0.63 bars
    'edge-nt-300x68x1028-act0-b11-beta-p4.8.4',          # 1.21 bars
    'edge-nt-300x68x516-act0-b10-p4.8.4-o100',          # 1.42 bars
    'edge-nt-300x68x516-act0-b10-p4.8.4-o010',          # 1.42 bars
    'edge-nt-300x68x516-act0-b10-p4.8.4-o001',          # 1.42 bars
    'edge-nn-45x70x1000-act0-b10-p3.2.3',          # 1.42 bars
    'edge-tn-45x70x1000-act0-b10-p3.2.3',          # 1.29 bars
    'edge-tn-38x68x523-act0-b10-p4.8.4',          # 1.42 bars
    'edge-nt-1x68x200-act1-b11-p4.8.4',          # 0.90 bars
    'edge-nn-1x68x200-act3-b10-beta-p4.8.4',          # 1.29 bars
    'edge-nn-32x68x200-act3-b10-beta-p4.8.4',          # 1.37 bars
    'edge-nt-31x127x200-act1-b11-p4.8.4',          # 1.41 bars
    'edge-nt-31x128x200-act1-b11-p4.8.4',          # 1.20 bars
    'edge-nn-31x128x200-act3-b10-beta-p4.8.4',          # 1.32 bars
    'edge-nt-31x129x131-act1-b11-p4.8.4',          # 1.26 bars
    'edge-nt-31x68x129-act1-b11-p4.8.4',          # 1.34 bars
    'edge-nn-31x68x129-act3-b10-beta-p4.8.4',          # 1.29 bars
    'edge-nt-31x68x160-act1-b11-p4.8.4',          # 1.45 bars
    'edge-nn-31x68x160-act3-b10-beta-p4.8.4',          # 1.24 bars
    'edge-nn-8x70x161-act3-b10-beta-p3.2.3',          # 1.36 bars
    'edge-nt-2047x70x20-act4-b10-beta-p4.8.4',          # 0.63 bars
    'edge-nt-2048x70x20-act4-b10-beta-p4.8.4',          # 0.55 bars
    'edge-nt-2049x70x20-act4-b10-beta-p4.8.4',          # 0.61 bars
    'edge-nt-2307x70x20-act4-b10-beta-p4.8.4',          # 0.60 bars
    'edge-nt-32x33x8192-act0-b10-p3.1.2',          # 1.06 bars
    'edge-nt-32x33x8192-act0-b11-beta-p4.8.4',          # 1.06 bars
    'edge-nn-32x33x8192-act0-b10-p3.1.2',          # 0.87 bars
    'edge-nn-32x33x8192-act0-b11-beta-p4.8.4',          # 0.87 bars
    'edge-nn-31x40x1200-act0-p4.0.0-skinny2-n1.9',          # 0.90 bars
    'edge-nn-8x64x8192-act0-p0.3.5-skinny2-n1.31',          # 0.80 bars
    'edge-tn-36x68x2059-act0-p4.8.4-tn_rows-map1030.1024.0.0',          # 0.96 bars
)
