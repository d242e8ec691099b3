"""NaN and +-inf through every activation epilogue and loss reduction, against the float64 references of tests/refs64_nonfinite.py, through
the C ABI.  The trainer's grad-norm gate sees a poisoned step only if a NaN that enters a layer is still a NaN when it leaves, so every row
of refs64_gemm.DENSE_CASES and refs64_conv.CONV_CASES runs once more on its own case with a NaN, +inf, -inf and a NaN in the last row or
pixel of the activations operand (refs64_nonfinite.poison_dense / poison_conv), with the runners of tests/test_dense_kernels_gpu.py and
tests/test_conv_kernels_gpu.py: the same buffers, guards, NaN prefill and canaries, the plan asserted before the launch.  Per row: the NaNs
and the signed infinities of the output are exactly where float64 has them, the finite elements are within the row's bar of the sibling
module, and a second run on fresh buffers gives the same bits on the finite part and the same pattern.  Rows too large for a float64
reference of the whole matrix compare the poisoned rows and the yardstick sample, and must be finite everywhere else.  The smallest row of
every epilogue site then runs with the other activations its entry point takes (refs64_nonfinite.dense_variants / conv_variants), the plan
asserted to stay on the site.  The Winograd families alone are held to the rule of
tests/test_kernels_gpu.py::test_conv_relu_propagates_nan_like_torch: what is non-finite in the reference is non-finite on the device, and the
device may add non-finite elements only inside the 2x2 output tiles (weight gradient: the output channels) that hold a poisoned input; outside
them the values are finite and within the bar.  The stand-alone kernels -- re2e_act_fwd (over more than one grid sweep and at n = 5),
re2e_act_bwd, re2e_act_bwd_colsum, re2e_fill_rows, re2e_loss_fwd / _bwd -- run on the small tables of the reference module.  GPU only.

Measured on an MI355X when the module was written.  Before the fixes that came with it (apply_act's ReLU was fmaxf(v, 0), the BCE logarithms
were clamped by fmaxf) 17 of the 245 cases failed, every one with the NaNs of the reference coming out as zeros (BCE: as 100 per element):
    test_dense_forms_keep_nan_and_inf[engine-nn-1-128x128x16-split-0-0-0-nn-45x68x520-act2-b10-beta-p4.8.4]
    test_dense_forms_keep_nan_and_inf[engine-nn-1-128x128x16-zx-0-0-0-nn-45x68x2056-act2-b11-p4.8.4]
    test_dense_forms_keep_nan_and_inf[engine-nn-0-32x128x32-zx-0-0-0-nn-8x70x522-act2-b10-p3.2.3]
    test_dense_forms_keep_nan_and_inf[engine-nt-1-128x128x16-one-0-0-0-nt-37x70x20-act2-b11-beta-p4.8.4]
    test_dense_forms_keep_nan_and_inf[engine-nt-0-32x128x32-split-0-0-0-nt-8x70x202-act2-b10-beta-p3.2.3]
    test_dense_forms_keep_nan_and_inf[engine-tn-0-128x128x16-zx-0-0-0-tn-37x70x2059-act2-b10-p3.2.3]
    test_dense_forms_keep_nan_and_inf[engine-nt-1-32x128x32-one-0-0-0-nt-8x24578x132-act2-b11-beta-p4.8.4]
    test_dense_sites_with_the_other_activations[engine_split-engine-nn-0-32x128x32-split-0-0-0-nn-8x70x202-act2-b11-p3.2.3]
    test_convolution_sites_with_the_other_activations[cin1_fwd-fwd-cin1_fwd-3x3-1x5x3-1to4-k3s1-act2]
    test_convolution_sites_with_the_other_activations[cout1_fixed_taps-fwd-cout1-16-3-3-1-1x5x3-64to1-k3s1-act2]
    test_convolution_sites_with_the_other_activations[cout1_generic-fwd-cout1-1-0-0-0-2x5x7-4to1-k3s1-act2]
    test_convolution_sites_with_the_other_activations[cout1_rows-fwd-cout1_rows-1x35x19-64to1-k3s1-act2]
    test_act_fwd_keeps_nan_and_inf[5]   test_act_fwd_keeps_nan_and_inf[4194317]   test_fill_rows_keeps_nan_and_inf
    test_losses_keep_nan_and_inf[BCE]   test_losses_keep_nan_and_inf[smoothL1]
that is the ReLU of the engine's epilogue with beta != 0 and of splitk_reduce_kernel (every split plan), of the three thin-convolution
kernels, of re2e_act_fwd and of re2e_fill_rows with a row_vec, the BCE value, and -- not foreseen -- the smooth-L1 GRADIENT, which was -1 at a
NaN difference where autograd gives NaN.  What passed before the fixes, although it calls apply_act: the pipeline -- its x W^T epilogue has
its own select, and the apply_act call of gemm_nt.hip sits in the x^T W form of the kernel, to which no entry point passes an activation; the
LeakyReLU of every site (v > 0 ? v : 0.2 v keeps a NaN and both infinities); relu_mask_kernel and the mk > 0 masks of conv3x3.hip /
winograd.hip (selects on a finite mask: a non-finite gradient passes or is zeroed as in threshold_backward); the L1 gradient (0 at a NaN,
as torch's sign).  With the fixes all 245 pass.  Poisoned cases per family, worst distance of the FINITE part from float64, then the bar:
    dense   skinny_wg     K <= 1024   5  1.85e-7  2e-6
            engine        K <= 1024  25  5.22e-7  2e-6
            engine_split  K <= 1024  23  7.14e-7  3e-6      K > 1024  12  4.67e-7  5e-6
            pipeline      K <= 1024  24  8.92e-7  2e-6      K > 1024   2  1.07e-6  4e-6
            mask          K <= 1024  12  1.05e-7  7e-7
    direct  y  39  5.61e-7  2e-6     dx  32  5.39e-7  2e-6     dW  27  5.27e-7  4e-6     pool  2  4.11e-7  2e-6
    wino3x3 y  20  4.36e-7  2e-6     dx   2  3.74e-7  2e-6     dW   5  6.52e-7  5e-6     pool  1  2.80e-7  3e-6
    wino4x4 y   1  2.21e-6  8e-6     dx   1  2.31e-6  1e-5     dW   2  1.37e-5  3e-5
    pointwise (activations, their backward, fill_rows, loss values)  48  1.34e-7  1e-5
The Winograd relaxation is used by the forward rows with a ReLU alone (F(2x2,3x3), 64 and 128 output channels: about 2900 non-finite elements
where float64 has 2300, ReLU(-inf) = 0 being a NaN inside a tile that holds the -inf) and by the pooled row; every other Winograd row has
exactly the reference's pattern.  The whole module takes 8 s.
"""
import pytest
import torch

import refs64_conv as C
import refs64_gemm as G
import refs64_nonfinite as R
import test_conv_kernels_gpu as K
import test_dense_kernels_gpu as D
from test_loss_kernels_gpu import DEV, _ops

pytestmark = pytest.mark.gpu

WORST = {}          # family -> [poisoned cases, worst finite distance from float64, bar]


def _note(key, err, bar):
    w = WORST.setdefault(key, [0, 0.0, bar])
    w[0] += 1
    w[1] = max(w[1], err)


def _guarded(fn, *args):
    """Nothing more is launched behind a device error (torch's report of a HIP fault), here or in tests/test_conv_kernels_gpu.py."""
    if K._DEVICE_ERROR:
        pytest.fail('not run: an earlier case ended in a device error (%s)' % K._DEVICE_ERROR[0])
    ops, lib = _ops()
    try:
        return fn(*args)
    except lib.Re2eError:
        raise
    except RuntimeError as e:
        K._DEVICE_ERROR.append('%s: %s' % (fn.__name__, str(e).splitlines()[0]))
        raise


def _same_bits(a, b, tag):
    fin = torch.isfinite(a)
    assert R.same_pattern(a, b) and torch.equal(a[fin].view(torch.int32), b[fin].view(torch.int32)), '%s: two runs on fresh buffers differ' % tag


# ---------------------------------------------------------------------------------------------
# dense products
# ---------------------------------------------------------------------------------------------
def _dense_check(row, site=None):
    ops, lib = _ops()
    tag = G.case_id(row)
    plan = D._device_plan(lib, row)
    key = G.family_of(row, plan)
    if row.entry != 'skinny2':          # the plan, first
        if not G.plan_matches(row.plan, plan) or key not in G.BARS:
            cus = torch.cuda.get_device_properties(0).multi_processor_count
            assert cus != 256, ('the plan drifted from what the row declares', tag, row.plan, plan)
            pytest.skip('the row declares its plan for a 256-CU chip; this one has %d CUs and plans %s' % (cus, plan))
        if row.form[0] != 'below_plan':
            assert G.form_key(plan, row) == row.form, (site, tag, plan)
    bar = G.BARS[key][0]
    clean = G.dense_case(row)
    case = R.poison_dense(row, clean)
    ref = R.dense_expected(row, case, clean)
    rows = torch.as_tensor(ref['rows'])
    st = None
    if row.filler:
        st = torch.cuda.Stream()
        lib.set_stream_role(st, True)
    try:
        def once():
            if st is None:
                got = D._run(lib, row, case)
            else:
                st.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(st):
                    got = D._run(lib, row, case)
                st.synchronize()
            if row.entry == 'nt_rows':          # the logical rows
                got['C'] = got['C'][case['map']]
            return got
        got, again = once(), once()
    finally:
        if st is not None:
            lib.set_stream_role(st, False)
    worst = 0.0
    for k in ('C', 'mask_out'):
        if k not in ref:
            continue
        sel = got[k][rows]
        differ = (torch.isnan(sel) != torch.isnan(ref[k])) | (torch.isposinf(sel) != torch.isposinf(ref[k])) | (torch.isneginf(sel) != torch.isneginf(ref[k]))
        assert R.same_pattern(sel, ref[k]), '%s %s: %d non-finite elements on the device, %d in float64; rows that differ: %s of the poisoned %s' % (
            tag, k, int((~torch.isfinite(sel)).sum()), int((~torch.isfinite(ref[k])).sum()), rows[differ.any(1)].tolist()[:8], [(p[0], p[1]) for p in case['poison']])
        rest = torch.ones(row.M, dtype=torch.bool)
        rest[rows] = False
        assert torch.isfinite(got[k][rest]).all(), '%s %s: a non-finite value outside the poisoned rows' % (tag, k)
        e = R.finite_err(sel, ref[k], ref['scale'])
        worst = max(worst, e)
        assert e <= bar, (tag, k, e, bar)
        _same_bits(got[k], again[k], tag + ' ' + k)
    print('NONFINITE %-96s %-22s finite part %.2e  bar %.0e  %d of %d rows compared' % (tag, '%s %s' % key, worst, bar, len(rows), row.M))
    _note('dense %s %s' % key, worst, bar)


@pytest.mark.parametrize('row', G.DENSE_CASES, ids=G.case_id)
def test_dense_forms_keep_nan_and_inf(row):
    _guarded(_dense_check, row)


@pytest.mark.parametrize('site,row', R.dense_variants(), ids=lambda v: v.replace(' ', '_') if isinstance(v, str) else G.case_id(v))
def test_dense_sites_with_the_other_activations(site, row):
    _guarded(_dense_check, row, site)


# ---------------------------------------------------------------------------------------------
# convolutions
# ---------------------------------------------------------------------------------------------
def _conv_check(row, variant=False):
    ops, lib = _ops()
    args, flags = C.plan_args(row)
    plan = lib.conv_plan(*args, flags=flags)
    got_form = C.form_key(row.direction, plan)
    assert R.same_site(row.form, got_form) if variant else got_form == row.form, plan
    fam = C.family_of(row, plan['family'])
    tag = '%s%s [%s]' % (C.case_id(row), ' act %d' % row.act if variant else '', '-'.join(str(v) for v in got_form))
    assert not row.flags & C.F_FILLER
    case = R.poison_conv(row, C.conv_case(row))
    ref = R.conv_expected(row, case)
    (out, idx), (out2, idx2) = K._once(lib, row, case, fam, plan, finite=False), K._once(lib, row, case, fam, plan, finite=False)
    _same_bits(out, out2, tag)
    assert idx is None or torch.equal(idx, idx2)
    pool = bool(row.flags & C.F_POOL)
    r64 = ref[0] if pool else ref
    q = C.quantity_of(row)
    bar = C.BARS[q, fam]
    bad64, bad = ~torch.isfinite(r64), ~torch.isfinite(out)
    if C.family_of(row) in ('wino3x3', 'wino4x4'):          # the one relaxation, for the families whose transforms mix the pixels of a tile
        assert fam == C.family_of(row)
        may = R.touched(row, case)
        assert bad[bad64].all(), '%s: %d elements that are NaN or infinite in float64 are finite on the device' % (tag, int((bad64 & ~bad).sum()))
        assert may[bad].all(), '%s: %d non-finite elements outside the tiles that hold a poisoned input' % (tag, int((bad & ~may).sum()))
    else:
        assert R.same_pattern(out, r64), '%s: %d non-finite elements on the device, %d in float64 (NaN %d / %d)' % (
            tag, int(bad.sum()), int(bad64.sum()), int(torch.isnan(out).sum()), int(torch.isnan(r64).sum()))
    e = R.finite_err(out, r64)
    assert e <= bar, '%s %s: the finite part is %.3e of the max from float64 (bar %.1e)' % (tag, q, e, bar)
    if pool:
        known = ~torch.isnan(r64) & ~torch.isnan(out)          # (an infinite maximum has its place like a finite one; a NaN window passes nothing back)
        assert torch.equal(idx[known], ref[1][known]) and (idx[torch.isnan(r64)] == 4).all(), '%s: index bytes' % tag
    if row.flags & C.F_MASK:
        assert (out[case['x'] == 0] == 0).all(), '%s: the gradient passes only where the ReLU output is > 0' % tag
    print('NONFINITE %-84s %-4s %-7s finite part %.2e  bar %.0e  non-finite %d (float64 %d) of %d' % (tag, q, fam, e, bar, int(bad.sum()), int(bad64.sum()), out.numel()))
    _note('%s %s' % (fam, q), e, bar)


@pytest.mark.parametrize('row', C.CONV_CASES, ids=C.case_id)
def test_convolution_forms_keep_nan_and_inf(row):
    _guarded(_conv_check, row)


@pytest.mark.parametrize('site,row', R.conv_variants(), ids=lambda v: v.replace(' ', '_') if isinstance(v, str) else '%s-act%d' % (C.case_id(v), v.act))
def test_convolution_sites_with_the_other_activations(site, row):
    _guarded(_conv_check, row, True)


# ---------------------------------------------------------------------------------------------
# the stand-alone kernels
# ---------------------------------------------------------------------------------------------
def _pointwise(tag, got, ref, bar, exact=False):
    """The pattern exactly, the finite part within ``bar`` of its max (exact: bit for bit)."""
    assert R.same_pattern(got, ref), '%s: NaN %d (float64 %d), inf %d (float64 %d)' % (
        tag, int(torch.isnan(got).sum()), int(torch.isnan(ref).sum()), int(torch.isinf(got).sum()), int(torch.isinf(ref).sum()))
    e = R.finite_err(got, ref)
    print('NONFINITE %-40s finite part %.2e  bar %.0e' % (tag, e, bar))
    assert e == 0.0 if exact else e <= bar, (tag, e, bar)
    _note('pointwise', e, bar)


@pytest.mark.parametrize('n', [5, 2 * 8192 * 256 + 13])
def test_act_fwd_keeps_nan_and_inf(n):
    _guarded(_act_fwd_keeps_nan_and_inf, n)


def _act_fwd_keeps_nan_and_inf(n):
    """re2e_act_fwd, the U-Net's stand-alone activations; the larger n is more than one sweep of its grid."""
    ops, lib = _ops()
    x = R.act_table(n)
    xd = K._in(x)
    for act in R.ACTS:
        y = K._Out((n,))
        lib.call('re2e_act_fwd', xd.data_ptr(), y.ptr(), n, act)
        _pointwise('act_fwd n=%d act=%d' % (n, act), y.result('act_fwd', finite=False), R.act_ref(x.double(), act), R.BAR_FBANK_OUT, exact=act == R.ACT_RELU)


@pytest.mark.parametrize('M,N', [(24, 16), (37, 10)], ids=['vectorised', 'scalar'])
def test_act_bwd_keeps_a_nonfinite_gradient(M, N):
    _guarded(_act_bwd_keeps_a_nonfinite_gradient, M, N)


def _act_bwd_keeps_a_nonfinite_gradient(M, N):
    """re2e_act_bwd and re2e_act_bwd_colsum (both of its paths) with a non-finite dy and a finite saved output."""
    ops, lib = _ops()
    dy, y = R.act_bwd_table(M, N)
    dyd, yd = K._in(dy), K._in(y)
    wsb = lib.query('re2e_colsum_workspace_bytes', M, N)
    for act in R.ACTS:
        dz64, cs64 = R.act_bwd_ref(dy, y, act)
        dz = K._Out((M, N))
        lib.call('re2e_act_bwd', dyd.data_ptr(), yd.data_ptr(), dz.ptr(), M * N, act)
        _pointwise('act_bwd %dx%d act=%d' % (M, N, act), dz.result('act_bwd', finite=False), dz64, R.BAR_FBANK_OUT)
        dz, cs = K._Out((M, N)), K._Out((N,))
        ws, _ = K._ws(wsb)
        lib.call('re2e_act_bwd_colsum', dyd.data_ptr(), yd.data_ptr(), dz.ptr(), M, N, act, cs.ptr(), 0.0, ws.data_ptr(), wsb)
        _pointwise('act_bwd_colsum dz %dx%d act=%d' % (M, N, act), dz.result('act_bwd_colsum dz', finite=False), dz64, R.BAR_FBANK_OUT)
        _pointwise('act_bwd_colsum sums %dx%d act=%d' % (M, N, act), cs.result('act_bwd_colsum sums', finite=False), cs64, R.BAR_FBANK_OUT)


def test_fill_rows_keeps_nan_and_inf():
    _guarded(_fill_rows_keeps_nan_and_inf)


def _fill_rows_keeps_nan_and_inf():
    """re2e_fill_rows with a row_vec: act(row_vec) in the listed rows, the others untouched."""
    ops, lib = _ops()
    N, ldc, nrows = 24, 28, 7
    v = R.fill_table(N)
    vd = K._in(v)
    rows = torch.tensor([5, 0, 6], dtype=torch.int32)
    rd = rows.to(DEV)
    prior = torch.randn(nrows, ldc, generator=torch.Generator().manual_seed(3))
    for act in (R.ACT_NONE,) + R.ACTS:
        c = K._Out((nrows, ldc), prior)
        lib.call('re2e_fill_rows', c.ptr(), ldc, N, rd.data_ptr(), len(rows), 0.0, vd.data_ptr(), act)
        got = c.result('fill_rows', finite=False)
        want = prior.double().clone()
        want[rows.long(), :N] = R.act_ref(v.double(), act)
        keep = torch.ones(nrows, ldc, dtype=torch.bool)
        keep[rows.long(), :N] = False
        assert torch.equal(got[keep], prior[keep]), 'fill_rows wrote outside its rows'
        _pointwise('fill_rows act=%d' % act, got, want, R.BAR_FBANK_OUT, exact=act in (R.ACT_NONE, R.ACT_RELU))


@pytest.mark.parametrize('kind', [R.L2, R.L1, R.SMOOTH_L1, R.BCE], ids=['L2', 'L1', 'smoothL1', 'BCE'])
def test_losses_keep_nan_and_inf(kind):
    _guarded(_losses_keep_nan_and_inf, kind)


def _losses_keep_nan_and_inf(kind):
    """re2e_loss_fwd / re2e_loss_bwd: a NaN (an infinite difference) comes out as NaN (inf) in the value, the gradient follows autograd
    (BCE: ATen's formula) element by element, and on finite inputs -- the BCE table holds a = 0 and a = 1 -- the -100 clamp still holds."""
    ops, lib = _ops()
    n = R.LOSS_N
    wsb = lib.query('re2e_reduce_workspace_bytes', n)
    for poison in ('finite', 'nan') + (('inf',) if kind != R.BCE else ()):
        a, t = R.loss_table(kind, poison)
        v64, g64 = R.loss_ref(kind, a, t)
        ad, td = K._in(a), K._in(t)
        ws, _ = K._ws(wsb)
        out, da = K._Out((1,)), K._Out((n,))
        lib.call('re2e_loss_fwd', ad.data_ptr(), td.data_ptr(), 0.0, n, kind, out.ptr(), ws.data_ptr(), wsb)
        lib.call('re2e_loss_bwd', ad.data_ptr(), td.data_ptr(), 0.0, n, kind, None, 1.0, da.ptr(), 0.0)
        tag = 'loss kind=%d %s' % (kind, poison)
        _pointwise(tag + ' value', out.result(tag, finite=False).view(()), v64, R.BAR_LOSS)
        got = da.result(tag, finite=False)
        assert R.same_pattern(got, g64), '%s gradient: NaN %d (float64 %d)' % (tag, int(torch.isnan(got).sum()), int(torch.isnan(g64).sum()))
        fin = torch.isfinite(g64)          # element by element: the BCE gradients span 1e-33 .. 1e12; 1 / n is the gradient of a unit slope
        tol = R.BAR_LOSS * (g64[fin].abs() + 1.0 / n)
        assert ((got[fin].double() - g64[fin]).abs() <= tol).all(), (tag, ((got[fin].double() - g64[fin]).abs() / tol).max().item())


def test_zz_worst_per_family():
    """Prints, per family, the number of poisoned cases that ran before it in this module and their worst finite distance from float64."""
    for key in sorted(WORST):
        n, e, bar = WORST[key]
        print('WORST %-22s %3d cases  finite part %.2e  bar %.0e' % (key, n, e, bar))
        assert e <= bar
