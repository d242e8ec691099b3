"""Pins tests/refs64_gemm.py (CPU only): the float64 dense reference against F.linear, ``@``, torch's activations, index_select and index_add on
doubles; that ``DENSE_CASES`` names exactly the kernel forms the dense plan (re2e_gemm_plan) can name on a 256-CU chip, every row with the plan
it declares, and that what is built and never named is ``NEVER_NAMED``; that the bars of tests/test_dense_kernels_gpu.py are what their rule
gives (8 x the worst distance of the fp32 CPU yardstick from float64 over every input of that test, rounded up to one significant digit, none
above 1e-5); that every input can SEE a wrong kernel (eleven deliberate mistakes in the reference, each on every row it applies to); and how
many shapes of the older dense tests of tests/test_kernels_gpu.py would have let each mistake pass.

The closure sweep below names 73 forms under refs64_gemm.form_key; DENSE_CASES holds 77 rows (two more on a filler stream, two for the forms
below the plan), NEVER_NAMED the four schedules of pipeline variant 3 that no shape reaches."""
import functools
import math
import os

import pytest
import torch
import torch.nn.functional as F

import refs64_gemm as R

ALL = list(R.DENSE_CASES) + list(R.EDGES)
_NT, _NN, _TN = (0, 1), (0, 0), (1, 0)
# what the dense entry points instantiate: tests/test_abi.py's copy of csrc/igemm.hip's tile table per form and VEC and of csrc/gemm_nt.hip's
# variant table, the four skinny_gemm_kernel<TB, VEC> instantiations, and the DenseMG pair of re2e_gemm_tn_rows (big_built<true>(true))
_SKINNY_BUILT = {('nt', 0), ('nt', 1), ('nn', 0), ('nn', 1)}
_DENSEMG_BUILT = {'128x128x16', '256x128x16'}


def _lib():
    from robust_e2e_gan_amd import lib
    if not os.path.exists(lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return lib


def _plan(row):
    if row.entry == 'skinny2':
        return R.SKINNY2_PLAN
    args, kw = R.plan_args(row)
    return _lib().gemm_plan(*args, cus=256, **kw)


@functools.lru_cache(maxsize=None)
def _measured(i):
    """-> (plan, BARS key, float64 reference on the yardstick rows, distance of the fp32 'mm' yardstick from it, of the 'k2' yardstick)."""
    row = ALL[i]
    plan = _plan(row)
    key = R.family_of(row, plan)
    case = R.dense_case(row)
    rows = R.yard_rows(row) or list(range(row.M))
    ref = R.dense_ref(row, case, rows=rows, plan=plan)
    e = {o: R.dense_err(R.dense_ref(row, case, torch.float32, order=o, rows=rows, plan=plan), ref) for o in ('mm', 'k2')}
    return plan, key, ref, e['mm'], e['k2']


# ---------------------------------------------------------------------------------------------
# pinning
# ---------------------------------------------------------------------------------------------
_ACTS = {R.ACT_NONE: lambda t: t, R.ACT_TANH: torch.tanh, R.ACT_RELU: F.relu, R.ACT_LRELU: lambda t: F.leaky_relu(t, 0.2), R.ACT_SIGMOID: torch.sigmoid}


@pytest.mark.parametrize('M,N,K', [(7, 5, 3), (37, 70, 21), (1, 1, 1), (33, 4, 130)])
def test_reference_is_linear_and_matmul_in_double(M, N, K):
    for act, fn in _ACTS.items():
        for beta in (0, 1):
            row = R._row(None, 'nt', M, N, K, act=act, bias2=1, beta=beta)
            c = {k: (v.double() if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in R.dense_case(row).items()}
            want = fn(F.linear(c['A'], c['B'], c['b1'] + c['b2'])) + beta * c['C0']          # the activation BEFORE the beta term
            got = R.dense_ref(row, c)
            assert R.rel_err(got['C'], want) <= 1e-12 and abs(got['scale'] - (c['A'] @ c['B'].t()).abs().max().item()) <= 1e-12 * got['scale']
            row = R._row(None, 'nn', M, N, K, act=act, bias=0, beta=beta)
            c = {k: (v.double() if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in R.dense_case(row).items()}
            assert R.rel_err(R.dense_ref(row, c)['C'], fn(c['A'] @ c['B']) + beta * c['C0']) <= 1e-12
            row = R._row(None, 'tn', M, N, K, act=act, bias2=1, beta=beta)          # (re2e_gemm takes the biases in every operand form)
            c = {k: (v.double() if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in R.dense_case(row).items()}
            assert R.rel_err(R.dense_ref(row, c)['C'], fn(c['A'].t() @ c['B'] + c['b1'] + c['b2']) + beta * c['C0']) <= 1e-12
    row = R._row(None, 'nn', M, N + 3, K, entry='skinny2', n1=3, plan=R.SKINNY2_PLAN)
    c = R.dense_case(row)
    assert R.rel_err(R.dense_ref(row, c)['C'], c['A'].double() @ c['B'].double()) <= 1e-12


@pytest.mark.parametrize('rmap', [(5, 3, 0, 0), (0, 0, 1, 2), (20, 20, 0, 3), (11, 0, 0, 1)])
def test_row_map_paths_are_index_arithmetic_in_double(rmap):
    Mv, N, K = 20, 6, 9
    row = R._row(None, 'nt', Mv, N, K, act=R.ACT_TANH, bias2=1, beta=1, entry='nt_rows', rmap=rmap)
    c = R.dense_case(row)
    m, phys = R.map_of(row)
    assert c['A'].shape[0] == phys == c['C0'].shape[0] and len(m) == Mv and len(set(m.tolist())) == Mv and int(m.max()) == phys - 1 - rmap[3]
    assert (m[:rmap[0]] == torch.arange(rmap[0])).all() or rmap[2]
    want = c['C0'].double().clone()
    x = c['A'].double().index_select(0, m)
    want.index_copy_(0, m, torch.tanh(F.linear(x, c['B'].double(), c['b1'].double() + c['b2'].double())) + c['C0'].double().index_select(0, m))
    got = R.dense_ref(row, c)['C']
    assert R.rel_err(got, want) <= 1e-12
    out = torch.ones(phys, dtype=torch.bool)
    out[m] = False
    assert torch.equal(got[out], c['C0'].double()[out]), 'rows outside the map are untouched'
    poisoned = dict(c, A=c['A'].clone())
    poisoned['A'][out] = float('nan')
    assert torch.equal(R.dense_ref(row, poisoned)['C'], got), 'rows outside the map are not read'
    # x^T W: the contraction walks the map only
    row = R._row(None, 'tn', 7, N, Mv, beta=1, entry='tn_rows', rmap=rmap)
    c = R.dense_case(row)
    m, phys = R.map_of(row)
    dy = torch.zeros(phys, 7, dtype=torch.float64).index_add_(0, m, c['A'].double().index_select(0, m))          # dy with zeros in the padded rows
    want = dy.t() @ torch.nan_to_num(c['B'].double()) + c['C0'].double()
    got = R.dense_ref(row, c)['C']
    assert R.rel_err(got, want) <= 1e-12
    out = torch.ones(phys, dtype=torch.bool)
    out[m] = False
    poisoned = dict(c, A=c['A'].clone(), B=c['B'].clone())
    poisoned['A'][out] = float('nan')
    poisoned['B'][out] = float('nan')
    assert torch.equal(R.dense_ref(row, poisoned)['C'], got)


def test_mask_epilogue_is_sigmoid_times_length_mask_times_mul():
    T, lens = 5, (5, 1, 3)
    row = R._row(None, 'nt', 15, 6, 9, act=R.ACT_MASK, bias2=1, T=T, lens=lens)
    c = R.dense_case(row)
    got = R.dense_ref(row, c)
    live = (torch.arange(T)[None, :] < torch.tensor(lens)[:, None]).reshape(-1, 1).double()          # row = b T + t
    mask = torch.sigmoid(F.linear(c['A'].double(), c['B'].double(), c['b1'].double() + c['b2'].double())) * live
    assert R.rel_err(got['mask_out'], mask) <= 1e-12 and R.rel_err(got['C'], mask * c['mul'].double()) <= 1e-12
    assert (got['mask_out'][1 * T + 1:2 * T] == 0).all() and (got['mask_out'][:T] > 0).all()


def test_written_out_orders_are_the_product():
    g = torch.Generator().manual_seed(3)
    a, b = R.rnd(g, 9, 37), R.rnd(g, 37, 5)
    for sl in ([(0, 37)], [(0, 16), (16, 32), (32, 37)], [(0, 8), (8, 37)]):
        assert R.rel_err(R._mm_k2(a, b, sl), a.double() @ b.double()) <= 2e-6
    assert R.rel_err(R.round16(a), a) <= 2 ** -17 and R.rel_err(R.round11(a), a) <= 2 ** -12 and not torch.equal(R.round16(a), a)
    row = R._row(None, 'tn', 8, 4, 1000, plan=dict(route='engine', tile='128x128x16', splits='3'))
    assert R.k_slices(row, row.plan) == [(0, 336), (336, 672), (672, 1000)]          # 63 k-tiles of 16: 21 per slice
    row = R._row(None, 'nt', 8, 4, 72, plan=dict(route='skinny_wg'))
    assert R.k_slices(row, row.plan) == [(k, k + 16) for k in range(0, 64, 16)] + [(64, 72)]          # nine k-groups: two per wavefront, three idle


# ---------------------------------------------------------------------------------------------
# closure
# ---------------------------------------------------------------------------------------------
_MS = (1, 4, 8, 31, 32, 33, 36, 64, 255, 256, 257, 300, 1024, 2047, 2048, 2049, 4352, 6400, 7777, 12800)
_NS = (1, 4, 31, 32, 33, 64, 130, 255, 256, 257, 260, 512, 1024, 2046, 2048, 2049, 24578, 24580)
_KS = (4, 16, 63, 64, 127, 128, 260, 512, 1024, 2048, 4096, 4240, 8192, 8196, 12800)
_ALIGN = ((True, True, True), (True, True, False), (False, False, False), (True, False, False), (False, True, False))          # all, C unaligned, none, A only, B only
# what the fine sweep needed beyond the grid: whole tiles of variant 3, the all-tail schedule of variant 6, tails behind whole tiles
_FINE = ((2305, 1668, 20), (257, 5504, 3584), (3073, 2048, 260), (6400, 1024, 260), (12800, 132, 516), (7777, 260, 516), (7777, 260, 36))


def _sweep():
    """Operand forms x shapes x activations {none, tanh, mask} x alignment x entry point (re2e_gemm, the mapped one of the form) x
    stream role."""
    for op, (ta, tb) in R.TRANS.items():
        shapes = [(M, N, K) for M in _MS for N in _NS for K in _KS] + (list(_FINE) if op == 'nt' else [])
        for M, N, K in shapes:
            for act in (R.ACT_NONE, R.ACT_TANH, R.ACT_MASK):
                for al in _ALIGN:
                    for entry in ('gemm', op + '_rows'):
                        if entry == 'nn_rows' or (entry != 'gemm' and act == R.ACT_MASK) or (entry == 'nt_rows' and len(set(al)) > 1):
                            continue
                        for filler in (False, True):
                            yield (ta, tb, M, N, K), dict(act=act, aligned=al, rowmap=entry != 'gemm', filler=filler), R.Query(op, M, K, act, entry)


def _built_keys():
    """Every form_key the instantiations can carry: the engine's (form, vec, tile) x {one, split, zx}, the mask epilogue (a run-time branch of each of them) with one slice,
    the row tail of the 256x128 tile of x W^T, the DenseMG pair x {one, split, zx}; the pipeline's variants x schedules x row map; the skinny four."""
    import test_abi as T
    keys = {('skinny_wg', op, vec) for op, vec in _SKINNY_BUILT}
    keys |= {('pipeline', v, s, m) for v in T._PIPELINE_BUILT for s in ('dp', 'dp+sk', 'sk') for m in (0, 1)}
    for (form, vec), tiles in T._ENGINE_BUILT.items():
        op = R.OPS[form]
        for tile in tiles:
            keys |= {('engine', op, vec, tile, cls, 0, 0, 0) for cls in ('one', 'split', 'zx')}
            keys.add(('engine', op, vec, tile, 'one', 0, 1, 0))
    keys.add(('engine', 'nt', 1, '256x128x16', 'one', 1, 0, 0))
    keys |= {('engine', 'tn', 1, tile, cls, 0, 0, 1) for tile in _DENSEMG_BUILT for cls in ('one', 'split', 'zx')}
    return keys


def test_cases_are_closed_under_the_plans():
    """No device is touched (cus = 256).  Every form a plan names over the sweep has a row in DENSE_CASES and the other way round; every form is one
    of the instantiations that are built, and what is built and never named is NEVER_NAMED; every row's declared plan is what the library
    answers.  (The switch variables -- RE2E_NO_SKINNY_GEMM, RE2E_NT2, ... -- act in the experiments build only and are not swept.)"""
    lib = _lib()
    named, points = set(), 0
    for args, kw, q in _sweep():
        points += 1
        k = R.form_key(lib.gemm_plan(*args, cus=256, **kw), q)
        if k is not None:
            named.add(k)
    print('CLOSURE %d plans name %d forms' % (points, len(named)))
    declared = {row.form for row in R.DENSE_CASES if row.form[0] != 'below_plan'}
    assert named == declared, ('reachable without a numeric case', sorted(named - declared, key=str), 'declared and never named', sorted(declared - named, key=str))
    built = _built_keys()
    assert named <= built, sorted(named - built, key=str)
    assert built - named == set(R.NEVER_NAMED), (sorted(built - named - set(R.NEVER_NAMED), key=str), sorted(set(R.NEVER_NAMED) - (built - named), key=str))
    assert len(named) == 73 and points == 637466
    for row in ALL:
        plan = _plan(row)
        if row.entry == 'skinny2':
            assert row.M <= 32 and 0 < row.n1 < row.N
            continue
        got = R.form_key(plan, row)
        if row.form is None:          # an edge: it runs on the kernel family it declares
            assert got is not None and got not in R.NEVER_NAMED and R.plan_matches(row.plan, plan), (R.case_id(row), row.plan, plan)
            continue
        assert (('below_plan', 'fallback') + got if row.entry == 'gemm_nows' else got) == row.form, (R.case_id(row), got)
        assert R.plan_matches(row.plan, plan), (R.case_id(row), row.plan, plan)
    # the fallback row: its shape's own plan is the pipeline with a stream-K tail, and needs a workspace
    fb = [row for row in R.DENSE_CASES if row.entry == 'gemm_nows']
    assert len(fb) == 1
    p = lib.gemm_plan(0, 1, fb[0].M, fb[0].N, fb[0].K, act=fb[0].act, aligned=R.aligned_of(fb[0]), cus=256)
    assert p['route'] == 'pipeline' and int(p['g_sk']) > 0 and int(p['need']) > 0
    # stream roles: an engine row, a pipeline row and a mapped weight gradient run on a FILLER stream
    fill = {(row.form[0], row.entry) for row in R.DENSE_CASES if row.filler}
    assert {('engine', 'gemm'), ('pipeline', 'gemm'), ('engine', 'tn_rows')} <= fill
    ids = [R.case_id(row) for row in ALL]
    assert len(set(ids)) == len(ids)
    for fam in ('skinny_wg', 'pipeline', 'engine', 'engine_split', 'mask'):          # beta = 1 on at least one row per family (the mask epilogue has none)
        assert fam == 'mask' or any(row.beta for row in R.DENSE_CASES if R.family_of(row, _plan(row))[0] == fam), fam
    assert {row.act for row in R.DENSE_CASES} == set(range(6)) and all(row.pad[2] > 0 for row in R.DENSE_CASES)


# ---------------------------------------------------------------------------------------------
# bars and sensitivity
# ---------------------------------------------------------------------------------------------
def _round_up_one_digit(v):
    e = math.floor(math.log10(v))
    return math.ceil(v / 10 ** e - 1e-9) * 10 ** e


def test_bars_are_eight_times_the_worst_fp32_yardstick():
    worst = {}
    for i, row in enumerate(ALL):
        plan, key, _, e_mm, e_k2 = _measured(i)
        e = e_k2 if R.YARDSTICK[key[0]] == 'k2' else e_mm
        print('MARGIN %-92s %-22s fp32-cpu mm %.2e k2 %.2e  bar %.0e' % (R.case_id(row), '%s %s' % key, e_mm, e_k2, R.BARS[key][0]))
        assert e <= R.BARS[key][0] / 8, (R.case_id(row), e)
        worst[key] = max(worst.get(key, 0.0), e)
    for key, w in sorted(worst.items()):
        print('WORST %-28s %.3e -> bar %.0e' % ('%s %s' % key, w, R.BARS[key][0]))
        assert math.isclose(R.BARS[key][0], _round_up_one_digit(8 * w), rel_tol=1e-9), (key, w)
        assert math.isclose(R.BARS[key][1], w, rel_tol=5e-3), (key, w, 'the measured value written beside the bar')
    assert set(worst) == set(R.BARS) and max(b for b, _ in R.BARS.values()) <= R.BAR_CAP == 1e-5


@pytest.mark.parametrize('i', range(len(ALL)), ids=[R.case_id(row) for row in ALL])
def test_inputs_can_see_a_wrong_kernel(i):
    """Each of the mistakes (a)-(i) that applies to the row moves its output by more than 100 bars, operands of 11 mantissa bits by more than 10;
    operands of 16 mantissa bits (a two-term bf16 split) by more than 1.5 bars on exactly the rows that R.BLIND_TO_BF16X2 does not list."""
    row = ALL[i]
    plan, key, ref, _, _ = _measured(i)
    case = R.dense_case(row)
    rows = R.yard_rows(row) or list(range(row.M))
    bar = R.BARS[key][0]
    ms = R.mistakes_of(row, plan)
    assert {'a', 'c', 'j', 'k'} <= set(ms)
    for m in ms:
        e = R.dense_err(R.dense_ref(row, case, mistake=m, rows=rows, plan=plan), ref)
        print('SENSITIVITY %-92s (%s) %-66s %.1f bars' % (R.case_id(row), m, R.MISTAKES[m], e / bar))
        if m == 'k':
            assert (e > 1.5 * bar) == (R.case_id(row) not in R.BLIND_TO_BF16X2), (e / bar, 'R.BLIND_TO_BF16X2 lists the rows at or under 1.5 bars')
            assert e > bar or R.case_id(row) in R.BLIND_TO_BF16X2
        else:
            assert e > (10.0 if m == 'j' else 100.0) * bar, (m, R.MISTAKES[m], e / bar)


def test_every_mistake_has_a_row_and_the_short_rows_see_a_bf16_split():
    assert {m for i, row in enumerate(ALL) for m in R.mistakes_of(row, _measured(i)[0])} == set(R.MISTAKES)
    ids = {R.case_id(row): row for row in ALL}
    assert set(R.BLIND_TO_BF16X2) <= set(ids)
    short_blind = [i for i in R.BLIND_TO_BF16X2 if ids[i].K <= 1024]
    print('BF16X2 rows that would not tell a two-term bf16 split from fp32: %d of %d (K <= 1024: %d)' % (len(R.BLIND_TO_BF16X2), len(ALL), len(short_blind)))


# ---------------------------------------------------------------------------------------------
# what the older dense assertions of tests/test_kernels_gpu.py would have let pass
# ---------------------------------------------------------------------------------------------
# The calls of each older test as it makes them, (activation, bias, bias2, beta), and its tolerance in units of the largest |product|:
# test_gemm_nt_nn (1e-3 of the largest output), test_gemm_nt_pipeline_and_stream_k (2e-5), test_gemm_tn_splitk (2e-4), test_gemm_nt_rows and
# test_gemm_tn_rows (2e-5, through a row map), each at N(0, 1) operands as those tests draw them (so tanh sees pre-activations of sqrt(K)).
_NN_CALLS = ((R.ACT_TANH, 1, 0, 0), (R.ACT_NONE, 0, 0, 1))
_PIPE_CALLS = ((R.ACT_TANH, 1, 1, 0), (R.ACT_NONE, 0, 0, 1), (R.ACT_RELU, 0, 0, 1), (R.ACT_LRELU, 0, 0, 1), (R.ACT_SIGMOID, 0, 0, 1))
_OLD = ([('test_gemm_nt_nn', 'nt', M, N, K, _NN_CALLS, 1e-3, 0) for M, N, K in ((77, 257, 130), (256, 128, 64), (5, 3, 7), (300, 4233, 512), (130, 64, 257), (12800, 2048, 48), (12803, 2040, 36))] +
        [('test_gemm_nt_pipeline_and_stream_k', 'nt', M, N, K, _PIPE_CALLS, 2e-5, 0) for M, N, K in ((12288, 2048, 64), (12800, 512, 260), (6400, 512, 4240), (12800, 1024, 512), (2049, 260, 36),
                                                                                                   (7777, 1028, 1000), (300, 516, 200), (4100, 4, 20), (256, 64, 16), (25600, 256, 260))] +
        [('test_gemm_tn_splitk', 'tn', M, N, K, ((R.ACT_NONE, 0, 0, 1),), 2e-4, 0) for M, N, K in ((64, 96, 5000), (257, 130, 77), (1200, 812, 1312), (8, 4, 40000))] +
        [('test_gemm_nt_rows', 'nt', T * B, N, K, ((act, 1, 1, 0), (R.ACT_NONE, 0, 0, 1)), 2e-5, 1)
         for T, B, N, K, act in ((800, 32, 1024, 260, R.ACT_NONE), (200, 64, 512, 1024, R.ACT_TANH), (97, 24, 260, 36, R.ACT_RELU), (400, 16, 2048, 512, R.ACT_NONE))] +
        [('test_gemm_tn_rows', 'tn', M, N, T * B, ((R.ACT_NONE, 0, 0, 0), (R.ACT_NONE, 0, 0, 1)), 2e-5, 1) for T, B, M, N in ((800, 32, 1024, 260), (200, 64, 2048, 512), (97, 24, 132, 68), (300, 16, 512, 256))])


def test_old_assertions_pass_counts():
    """For each mistake but (i) (no older dense test runs the mask epilogue): on how many of the 29 shapes of the older dense tests the wrong result
    stays inside that test's own tolerance on EVERY call the test makes to which the mistake applies (shapes it applies to on no call are counted
    apart).  A CPU computation on 96 output rows of each shape (the first 48 and the last 48: mistakes b and c sit in the last row and columns),
    at most 512 columns and the first 12 800 k (the relative weight of one k, of a slice or of rounded operands does not grow with K), the
    mapped tests over 85 % of the rows, the split of (d) as the library plans the shape on 256 CUs; printed, for the commit message."""
    lib = _lib()
    counts, applies, per_test = {m: 0 for m in 'abcdefghjk'}, {m: 0 for m in 'abcdefghjk'}, {}
    for name, op, M, N, K, calls, tol, mapped in _OLD:
        Kc, Nc = min(K, 12800), min(N, 512)
        entry, rmap = 'gemm', None
        if mapped:          # the valid rows of a batch of lengths 0.7 T .. T: an identity prefix of 70 % of the physical rows, every second row behind it
            entry = op + '_rows'
            n = M if op == 'nt' else Kc
            M, Kc = (int(0.85 * n), Kc) if op == 'nt' else (M, int(0.85 * n))
            rmap = (int(0.7 * n), 0, 0, 0)
        ta, tb = R.TRANS[op]
        plan = lib.gemm_plan(ta, tb, M, Nc, Kc, rowmap=bool(mapped), cus=256)
        passed = {m: [] for m in counts}
        for act, bias, bias2, beta in calls:
            row = R._row(None, op, M, Nc, Kc, act=act, bias=bias, bias2=bias2, beta=beta, entry=entry, rmap=rmap)
            row = row._replace(bias=bias, bias2=bias2)          # (the mapped weight gradient takes none: its calls pass none)
            rows = sorted(set(range(min(48, M))) | set(range(max(0, M - 48), M)))
            case = R.dense_case(row)
            case['B'] = case['B'] * Kc ** 0.5          # N(0, 1), as the older tests draw their weights
            ref = R.dense_ref(row, case, rows=rows, plan=plan)
            for m in R.mistakes_of(row, plan):
                if m in counts:
                    passed[m].append(R.dense_err(R.dense_ref(row, case, mistake=m, rows=rows, plan=plan), ref) <= tol)
        for m, v in passed.items():
            if v:
                applies[m] += 1
                counts[m] += all(v)
                per_test.setdefault((name, m), []).append(all(v))
    for m in counts:
        print('OLD ASSERTIONS (%s) %-66s passes on %2d of the %2d shapes it applies to  [%s]' % (m, R.MISTAKES[m], counts[m], applies[m], ', '.join(
            '%s %d/%d' % (n.replace('test_gemm_', ''), sum(v), len(v)) for (n, mm), v in per_test.items() if mm == m)))
    assert counts['k'] == applies['k'] == len(_OLD), 'a two-term bf16 split passed every older assertion: the reason for this file'
    assert counts['j'] >= 7, 'operands of 11 mantissa bits passed test_gemm_nt_nn'
