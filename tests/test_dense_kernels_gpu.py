"""The dense product kernels -- csrc/igemm.hip's engine and skinny kernels, csrc/gemm_nt.hip's LDS-DMA pipeline with its stream-K tail, the
row-mapped entry points -- against the float64 reference of tests/refs64_gemm.py, through the C ABI (re2e_gemm, re2e_gemm_nt_rows,
re2e_gemm_tn_rows, re2e_gemm_skinny2), one row per kernel form the dense plan can name on a 256-CU chip plus the two forms below the plan
(the pipeline's run-time fallback to the engine, re2e_gemm_skinny2): every row of refs64_gemm.DENSE_CASES first asserts that the library's plan
on the device, for the row's alignment, row map and stream role, IS the plan the row declares, so a routing change cannot quietly empty a row
(tests/test_refs64_gemm_cpu.py checks that the table is closed under the plans).  A second test turns the edges (refs64_gemm.EDGES), each of which declares and first asserts the kernel family it is there for (route, pipeline
variant or engine tile, split or not); a third
the argument checks of the mapped entry points and of re2e_gemm_skinny2.

Every call: the operands sit in buffers of their leading dimensions in which every float outside the logical matrix is NaN (the columns behind
the widths, the physical rows a map leaves out); C (and mask_out) hold a known random canary in the columns N .. ldc and in the unmapped rows,
compared bit for bit afterwards, and the prior content beta = 1 adds on elsewhere.  The WHOLE output is held to the row's bar of
refs64_gemm.BARS -- 8 x the worst distance of the fp32 CPU yardstick from float64 per family and K class, none above 1e-5 -- in units of the
largest |op(A) op(B)|, and each row prints the HIP distance beside both fp32 CPU yardsticks.  Rows whose sum meets partial results (split-K,
XCD-ordered slices, a stream-K tail, the skinny kernels' eight wavefronts) run twice and must give the same bits.  Nothing here busies the
chip from a second stream: tests/test_kernels_gpu.py::test_gemm_nt_stream_k_tail_under_load keeps that job.  GPU only.

Measured on an MI355X when the module was written, worst case per family and K class over all 313 rows, HIP / fp32 'mm' yardstick on the CPU (of
the largest |op(A) op(B)|), then the bar:
    skinny_wg     K <= 1024  1.92e-7 / 1.80e-7  2e-6      K > 1024  1.03e-6 / 5.39e-7  5e-6   (K = 8192)
    pipeline      K <= 1024  9.03e-7 / 2.14e-7  2e-6      K > 1024  1.58e-6 / 4.26e-7  4e-6   (12800 x 132 x 516, variant 8, whole tiles + tail; 257 x 5504 x 3584 mapped)
    engine        K <= 1024  5.26e-7 / 1.70e-7  2e-6                                          (the run-time fallback row, 7777 x 260 x 516 on 256x128 tiles)
    engine_split  K <= 1024  7.14e-7 / 2.66e-7  3e-6      K > 1024  4.67e-7 / 5.97e-7  5e-6
    mask          K <= 1024  1.05e-7 / 8.57e-8  7e-7                                          (x W with the 32x128 tile; the epilogue runs on all three operand forms)
No family needed the strictly sequential 'k2' yardstick: the pipeline, which walks a contraction in one accumulator, is the farthest from the
pairwise order at 4.2 x and stays under half its bar.
"""
import functools

import pytest
import torch

import refs64_gemm as R
from test_loss_kernels_gpu import DEV, _ops

pytestmark = pytest.mark.gpu

NAN = float('nan')
SLACK = 8          # floats behind every buffer (canary / NaN), and room for a base one float behind a 16-byte boundary
WORST = {}         # BARS key -> (HIP distance, case id): printed by the last test of the module


@functools.lru_cache(maxsize=2)
def _refs(row):
    """Inputs and float64 reference of a row; rows that differ in what does not enter them (stream role, paddings, offsets, ident_rows, the
    declared plan) share both."""
    case = R.dense_case(row)
    return case, R.dense_ref(row, case, plan=R.SKINNY2_PLAN)          # (float64 and no mistake: the plan is not read)


def _key(row):
    """The part of a row its inputs and its float64 reference depend on."""
    rmap = None if row.rmap is None else (row.rmap[0], 0, row.rmap[2], row.rmap[3])
    return row._replace(form=None, plan=None, filler=False, pad=(0, 0, 0), off=(0, 0, 0), rmap=rmap)


def _buf(rows, width, ld, off, fill, content=None):
    """A device buffer of rows x ld floats (+ SLACK) whose base sits ``off`` floats behind a 16-byte boundary, prefilled with ``fill`` (NaN, or a
    CPU tensor of canary values of the same size), the logical rows x width matrix set to ``content`` -> (the flat store, the base address)."""
    n = rows * ld + SLACK
    host = torch.full((n,), NAN) if fill is None else fill.reshape(-1)[:n].clone()
    assert host.numel() == n
    if content is not None:
        host[off:off + rows * ld].view(rows, ld)[:, :width] = content
    store = host.to(DEV)
    assert store.data_ptr() % 16 == 0
    return store, store.data_ptr() + 4 * off


def _canary(n, seed):
    return torch.randn(n, generator=torch.Generator().manual_seed(seed))


def _run(lib, row, case=None):
    """One call of the row's entry point on fresh buffers -> dict(C=(physical rows, N) [, mask_out]) on the CPU, after the canary checks.
    case: other inputs of the row's shape than its own (tests/test_nonfinite_kernels_gpu.py)."""
    if case is None:
        case, _ = _refs(_key(row))
    M, N, K = row.M, row.N, row.K
    lda, ldb, ldc = R.leading_dims(row)
    oa, ob, oc = row.off
    ta, tb = R.TRANS[row.op]
    rows_a = case['A'].shape[0]
    A = case['A']
    Bm = case['B']
    if case['map'] is not None:          # NaN in the physical rows the map leaves out
        out = torch.ones(case['phys'], dtype=torch.bool)
        out[case['map']] = False
        A = A.clone()
        A[out] = NAN
        if row.entry == 'tn_rows':
            Bm = Bm.clone()
            Bm[out] = NAN
    wa, wb, wc = R.widths(row)
    rows_c = case['C0'].shape[0]
    b1 = case['b1'].to(DEV) if row.bias else None
    b2 = case['b2'].to(DEV) if row.bias2 else None
    p = lambda t: None if t is None else t.data_ptr()
    if row.entry == 'skinny2':
        n1, n2 = row.n1, N - row.n1
        sa, pa = _buf(M, K, lda, oa, None, A)
        sb1, pb1 = _buf(K, n1, n1 + row.pad[1], ob, None, Bm[:, :n1])
        sb2, pb2 = _buf(K, n2, n2 + row.pad[1], ob, None, Bm[:, n1:])
        can1, can2 = _canary(M * (n1 + row.pad[2]) + SLACK, 11), _canary(M * (n2 + row.pad[2]) + SLACK, 12)
        sc1, pc1 = _buf(M, n1, n1 + row.pad[2], oc, can1)
        sc2, pc2 = _buf(M, n2, n2 + row.pad[2], oc, can2)
        lib.call('re2e_gemm_skinny2', M, K, pa, lda, pb1, n1 + row.pad[1], n1, pc1, n1 + row.pad[2], pb2, n2 + row.pad[1], n2, pc2, n2 + row.pad[2])
        torch.cuda.synchronize()
        parts = []
        for store, can, n, tag in ((sc1, can1, n1, 'C1'), (sc2, can2, n2, 'C2')):
            parts.append(_split(store.cpu(), can, M, n, n + row.pad[2], oc, None, tag))
        return dict(C=torch.cat(parts, 1))
    sa, pa = _buf(rows_a, wa, lda, oa, None, A)
    sb, pb = _buf(Bm.shape[0], wb, ldb, ob, None, Bm)
    can_c = _canary(rows_c * ldc + SLACK, 13)
    sc, pc = _buf(rows_c, wc, ldc, oc, can_c, case['C0'])
    can_c[oc:oc + rows_c * ldc].view(rows_c, ldc)[:, :N] = case['C0']          # (what an untouched row of C still holds)
    extra = {}
    if row.entry == 'gemm_nows':
        ws, wsb = None, 0
    else:
        wsb = lib.query('re2e_gemm_workspace_bytes', ta, tb, M, N, K)
        ws = torch.full((wsb // 4 + 16,), NAN, device=DEV) if wsb else None
    if row.entry in ('gemm', 'gemm_nows'):
        mul = mask = lens = None
        if row.act == R.ACT_MASK:
            smul, pmul = _buf(M, N, ldc, oc, None, case['mul'])
            can_m = _canary(M * ldc + SLACK, 14)
            smask, pmask = _buf(M, N, ldc, oc, can_m, case['mask0'])
            can_m[oc:oc + M * ldc].view(M, ldc)[:, :N] = case['mask0']
            lens = case['lens'].to(torch.int32).to(DEV)
            extra = dict(mul=pmul, mask=pmask)
        lib.call('re2e_gemm', ta, tb, M, N, K, pa, lda, pb, ldb, pc, ldc, p(b1), p(b2), row.act, float(row.beta), extra.get('mul'), extra.get('mask'),
                 p(lens), row.T, p(ws), wsb)
    else:
        rmap = case['map'].to(torch.int32).to(DEV)
        if row.entry == 'nt_rows':
            ok = lib.call_supported('re2e_gemm_nt_rows', M, N, K, pa, lda, pb, ldb, pc, ldc, p(b1), p(b2), row.act, float(row.beta), rmap.data_ptr(), row.rmap[1],
                                    case['phys'], p(ws), wsb)
        else:
            ok = lib.call_supported('re2e_gemm_tn_rows', M, N, K, pa, lda, pb, ldb, pc, ldc, float(row.beta), rmap.data_ptr(), row.rmap[1], case['phys'], p(ws), wsb)
        assert ok, 'the mapped entry point declined a shape whose plan it runs'
    torch.cuda.synchronize()
    written = case['map'] if row.entry == 'nt_rows' else None
    got = dict(C=_split(sc.cpu(), can_c, rows_c, N, ldc, oc, written, 'C'))
    if row.act == R.ACT_MASK:
        got['mask_out'] = _split(smask.cpu(), can_m, M, N, ldc, oc, None, 'mask_out')
    return got


def _split(store, canary, rows, N, ld, off, written, tag):
    """The logical rows x N matrix of a C buffer read back, after checking bit for bit that everything else still holds the canary: the floats in
    front of the base and behind the last row, the columns N .. ld, and (written: the map) the rows outside the map."""
    body = store[off:off + rows * ld].view(rows, ld)
    want = canary[off:off + rows * ld].view(rows, ld)
    assert torch.equal(store[:off], canary[:off]) and torch.equal(store[off + rows * ld:], canary[off + rows * ld:]), '%s: wrote outside the buffer\'s rows' % tag
    assert torch.equal(body[:, N:].contiguous().view(torch.int32), want[:, N:].contiguous().view(torch.int32)), '%s: wrote beyond the N columns' % tag
    if written is not None:
        out = torch.ones(rows, dtype=torch.bool)
        out[written] = False
        assert torch.equal(body[out][:, :N].contiguous().view(torch.int32), want[out][:, :N].contiguous().view(torch.int32)), '%s: a row outside the map was touched' % tag
    return body[:, :N].clone()


def _device_plan(lib, row):
    if row.entry == 'skinny2':
        return R.SKINNY2_PLAN
    args, kw = R.plan_args(row)
    return lib.gemm_plan(*args, cus=0, **kw)


def _check(row):
    ops, lib = _ops()
    plan = _device_plan(lib, row)
    key = R.family_of(row, plan)
    if row.entry != 'skinny2':          # 1. the plan, first: a table row declares its whole plan, an edge its kernel family
        if not R.plan_matches(row.plan, plan) or key not in R.BARS:
            cus = torch.cuda.get_device_properties(0).multi_processor_count
            assert cus != 256, ('the plan drifted from what the row declares', R.case_id(row), row.plan, plan)
            pytest.skip('the row declares its plan for a 256-CU chip; this one has %d CUs and plans %s' % (cus, plan))
        if row.entry == 'gemm_nows':          # the shape's own plan is the pipeline with a stream-K tail: without a workspace it falls to the engine plan above
            own = lib.gemm_plan(0, 1, row.M, row.N, row.K, act=row.act, aligned=R.aligned_of(row), cus=0)
            assert own['route'] == 'pipeline' and int(own['g_sk']) > 0, own
    bar = R.BARS[key][0]
    st = None
    if row.filler:
        st = torch.cuda.Stream()
        lib.set_stream_role(st, True)
    try:
        def once():
            if st is None:
                return _run(lib, row)
            st.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(st):
                got = _run(lib, row)
            st.synchronize()
            return got
        got = once()
        case, ref = _refs(_key(row))
        e = R.dense_err(got, ref)
        rows = R.yard_rows(row) or list(range(row.M))
        r64 = R.dense_ref(row, case, rows=rows, plan=plan)
        yard = {o: R.dense_err(R.dense_ref(row, case, torch.float32, order=o, rows=rows, plan=plan), r64) for o in ('mm', 'k2')}
        print('DENSE %-92s %-22s HIP %.2e  fp32-cpu mm %.2e k2 %.2e  bar %.0e  %s' % (R.case_id(row), '%s %s' % key, e, yard['mm'], yard['k2'], bar,
                                                                                    ' '.join('%s=%s' % kv for kv in plan.items() if kv[0] not in ('ws', 'need'))))
        if e > WORST.get(key, (0.0, ''))[0]:
            WORST[key] = (e, R.case_id(row))
        assert e <= bar, (R.case_id(row), e, bar)
        twice = row.entry == 'skinny2' or plan['route'] == 'skinny_wg' or (plan['route'] == 'engine' and int(plan['splits']) > 1) or \
            (plan['route'] == 'pipeline' and int(plan['g_sk']) > 0)
        if twice:
            again = once()
            for k in got:
                assert torch.equal(got[k].view(torch.int32), again[k].view(torch.int32)), '%s differs between two identical calls: the arrival order matters' % k
    finally:
        if st is not None:
            lib.set_stream_role(st, False)


@pytest.mark.parametrize('row', R.DENSE_CASES, ids=R.case_id)
def test_dense_forms(row):
    _check(row)


@pytest.mark.parametrize('row', R.EDGES, ids=R.case_id)
def test_dense_edges(row):
    _check(row)


def _raw(lib, name, *args):
    return getattr(lib.load(), name)(*args, lib.stream())


def test_mapped_entry_points_refuse_what_they_do_not_run():
    """Argument checks: nothing is launched, C comes back bit-unchanged.  re2e_gemm_nt_rows on shapes whose plan is not the pipeline (fewer than
    256 mapped rows; N no multiple of 4; an unaligned A); re2e_gemm_tn_rows with Kv < 64 and with an unaligned operand; re2e_gemm without
    a workspace where both the pipeline's plan and the engine's need one; re2e_gemm_skinny2 with 33 rows."""
    ops, lib = _ops()
    so = lib.load()

    def untouched(store, canary):
        torch.cuda.synchronize()
        return torch.equal(store.cpu().view(torch.int32), canary.view(torch.int32))

    for Mv, N, K, off in ((200, 68, 36, 0), (300, 70, 36, 0), (300, 68, 36, 1)):
        row = R._row(None, 'nt', Mv, N, K, entry='nt_rows', rmap=(10, 0, 0, 0), off=(off, 0, 0), pad=(4, 8, 4) if N % 4 == 0 else (4, 8, 2))
        args, kw = R.plan_args(row)
        assert lib.gemm_plan(*args, cus=0, **kw)['route'] != 'pipeline'
        case = R.dense_case(row)
        lda, ldb, ldc = R.leading_dims(row)
        sa, pa = _buf(case['phys'], K, lda, off, None, case['A'])
        sb, pb = _buf(N, K, ldb, 0, None, case['B'])
        can = _canary(case['phys'] * ldc + SLACK, 5)
        sc, pc = _buf(case['phys'], N, ldc, 0, can)
        rmap = case['map'].to(torch.int32).to(DEV)
        ws = torch.zeros(1 << 20, device=DEV)
        rc = _raw(lib, 're2e_gemm_nt_rows', Mv, N, K, pa, lda, pb, ldb, pc, ldc, None, None, R.ACT_NONE, 0.0, rmap.data_ptr(), 0, case['phys'], ws.data_ptr(), ws.numel() * 4)
        assert rc == lib.EUNSUPPORTED and so.re2e_last_error(), (Mv, N, K, off, rc)
        assert untouched(sc, can), 'a refused call wrote C'
    for M, N, Kv, off in ((36, 68, 63, (0, 0, 0)), (36, 68, 70, (1, 0, 0)), (36, 68, 70, (0, 1, 0)), (38, 68, 70, (0, 0, 0))):
        row = R._row(None, 'tn', M, N, Kv, entry='tn_rows', rmap=(10, 0, 0, 0), off=off)
        case = R.dense_case(row)
        lda, ldb, ldc = R.leading_dims(row)
        sa, pa = _buf(case['phys'], M, lda, off[0], None, case['A'])
        sb, pb = _buf(case['phys'], N, ldb, off[1], None, case['B'])
        can = _canary(M * ldc + SLACK, 6)
        sc, pc = _buf(M, N, ldc, 0, can)
        rmap = case['map'].to(torch.int32).to(DEV)
        ws = torch.zeros(1 << 20, device=DEV)
        rc = _raw(lib, 're2e_gemm_tn_rows', M, N, Kv, pa, lda, pb, ldb, pc, ldc, 0.0, rmap.data_ptr(), 0, case['phys'], ws.data_ptr(), ws.numel() * 4)
        assert rc == lib.EUNSUPPORTED, (M, N, Kv, off, rc)
        assert untouched(sc, can), 'a refused call wrote C'
    # the run-time fallback of re2e_gemm on a shape whose ENGINE plan is split: no workspace, no product -- an error code, C untouched
    row = R._row(None, 'nt', 300, 68, 516, entry='gemm_nows')
    args, kw = R.plan_args(row)
    assert int(lib.gemm_plan(*args, cus=0, **kw)['splits']) > 1 and int(lib.gemm_plan(0, 1, 300, 68, 516, cus=0)['g_sk']) > 0
    case = R.dense_case(row)
    lda, ldb, ldc = R.leading_dims(row)
    sa, pa = _buf(300, 516, lda, 0, None, case['A'])
    sb, pb = _buf(68, 516, ldb, 0, None, case['B'])
    can = _canary(300 * ldc + SLACK, 8)
    sc, pc = _buf(300, 68, ldc, 0, can)
    rc = _raw(lib, 're2e_gemm', 0, 1, 300, 68, 516, pa, lda, pb, ldb, pc, ldc, None, None, R.ACT_NONE, 0.0, None, None, None, 0, None, 0)
    assert rc not in (0, lib.EUNSUPPORTED) and b'workspace' in so.re2e_last_error(), rc
    assert untouched(sc, can), 'a refused call wrote C'
    A, B1, B2 = torch.zeros(33, 64, device=DEV), torch.zeros(64, 8, device=DEV), torch.zeros(64, 8, device=DEV)
    can = _canary(33 * 8, 7)
    C1, C2 = can.to(DEV), can.to(DEV)
    rc = _raw(lib, 're2e_gemm_skinny2', 33, 64, A.data_ptr(), 64, B1.data_ptr(), 8, 8, C1.data_ptr(), 8, B2.data_ptr(), 8, 8, C2.data_ptr(), 8)
    assert rc != 0 and b'32' in so.re2e_last_error(), rc
    assert untouched(C1, can) and untouched(C2, can)
    with pytest.raises(lib.Re2eError):
        lib.call('re2e_gemm_skinny2', 33, 64, A.data_ptr(), 64, B1.data_ptr(), 8, 8, C1.data_ptr(), 8, B2.data_ptr(), 8, 8, C2.data_ptr(), 8)


def test_zz_worst_per_family():
    """Prints the worst HIP distance per family and K class over the rows that ran before it in this module (for DESIGN.md section 4.1)."""
    for key in sorted(WORST):
        e, cid = WORST[key]
        print('WORST %-28s HIP %.2e  fp32-cpu %.2e  bar %.0e  (%s)' % ('%s %s' % key, e, R.BARS[key][1], R.BARS[key][0], cid))
        assert e <= R.BARS[key][0]
