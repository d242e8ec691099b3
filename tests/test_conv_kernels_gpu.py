"""The convolution kernels -- csrc/igemm.hip, gemm_nt.hip, conv3x3.hip, thinconv.hip, winograd.hip, wino_wgrad.hip, wino44.hip -- against the
float64 reference of tests/refs64_conv.py, through the C ABI (re2e_conv_igemm, _masked, re2e_conv3x3_relu_pool, re2e_conv_dgrad_s2,
re2e_conv_wgrad, re2e_conv3x3_wino, _wino_wgrad, re2e_conv4x4_wino, _wino_wgrad), one row per kernel form the convolution plans can name on a
256-CU chip and per sub-form the Winograd files branch on below the plan: every row of refs64_conv.CONV_CASES first asserts that the library's
plan for its layer IS the form the row declares, so a routing change cannot quietly empty a row (tests/test_refs64_conv_cpu.py checks that
the table is closed under the plans).  A second test turns the edges (refs64_conv.EDGES), a third runs whole layers through ops.conv2d /
ops.conv_transpose2d and autograd.

Every call: outputs and workspaces are prefilled with NaN (beta = 1: with the tensor to accumulate on), each output sits between guard floats
inside one allocation, which must come back bit-unchanged; the call runs twice on fresh buffers and the two results must be equal bit for
bit.  Results are held to the bars of refs64_conv.BARS -- 8 x the worst distance of the fp32 CPU yardstick from float64, per quantity and
family, none above 5e-5 -- and each row prints the HIP and the fp32 CPU distance.  A pooled forward is checked in its values and its index
bytes: an index may differ from the float64 one only between window entries that float64 itself holds closer than the bar.  GPU only.

Measured on an MI355X when the module was written, worst case per family and quantity over the 353 checked tensors, HIP / fp32 yardstick on the
CPU (of the tensor's max), then the bar:
    direct    y    1.76e-6 / 1.95e-7   2e-6     (pipeline 128x64x16, 4x4 / stride 2, 64 -> 128: a contraction of 1024 terms; next 1.0e-6 at 576)
              dx   1.32e-6 / 2.03e-7   2e-6     (halo 16x16 as a data gradient, 128 -> 64 channels: 1152 terms)
              dW   7.2e-7  / 4.5e-7    4e-6     (every wide_reduce = 1 row <= 3.9e-7; unaligned 64 -> 64 worst)
              db   2.1e-7  / 1.1e-7    9e-7
              pool 5.2e-7  / 1.4e-7    2e-6     (index bytes equal to the float64 ones on every row)
    wino3x3   y    4.9e-7  / 2.1e-7    2e-6       dx 7.2e-7 / 2.0e-7  2e-6       dW 6.5e-7 / 5.5e-7  5e-6       pool 3.6e-7 / 3.0e-7  3e-6
    wino4x4   y    2.6e-6  / 9.2e-7    8e-6       dx 3.0e-6 / 1.1e-6  1e-5       dW 1.4e-5 / 3.4e-6  3e-5  (sub = 1: 1.4e-5, sub = 2 over padded tiles: 1.0e-5)
The thin kernels and the engine sit at 1 - 3 x the yardstick.  The matrix-core kernels that walk the whole contraction in one accumulator (halo,
pipeline) grow with its length as a sequential fp32 sum does -- 5e-7 at 144 terms, 1.0e-6 at 576, 1.8e-6 at 1024, up to 10 x a yardstick that
sums blocks of 32 pairwise -- and stay inside the bars at every shape of these tables; nothing points at products of fewer than 24 bits.
"""
import functools

import pytest
import torch

import refs64_conv as R
from test_loss_kernels_gpu import DEV, _ops

pytestmark = pytest.mark.gpu

NAN = float('nan')
GUARD, PATTERN = 64, 1234.5          # floats (256 bytes: the output stays 16-byte aligned) before and after every output


@functools.lru_cache(maxsize=None)
def _refs(row, fam):
    """Inputs, float64 reference and fp32 CPU yardstick of a row; rows that differ in what does not enter them (stream role, alignment, the
    family's switches) share all three."""
    case = R.conv_case(row)
    return case, R.case_ref(row, case), R.case_yardstick(row, case, fam)


def _key(row):
    """The part of a row its inputs and its reference depend on."""
    keep = R.F_BIAS | R.F_POOL | R.F_MASK
    return row._replace(form=None, sub=None, via=None, flags=row.flags & keep)


class _Out(object):
    """A device output of n elements between two guards, inside one allocation; off16: 4 bytes off a 16-byte boundary (float outputs)."""

    def __init__(self, shape, init=None, off16=False, dtype=torch.float32):
        n = 1
        for v in shape:
            n *= v
        self.byte = dtype == torch.uint8
        self.fill = 0xAB if self.byte else PATTERN
        self.off = GUARD + (1 if off16 else 0)
        self.n = n
        self.store = torch.full((n + 2 * GUARD + 4,), self.fill, dtype=dtype, device=DEV)
        self.t = self.store[self.off:self.off + n].view(shape)
        if init is None:
            self.t.fill_(0xFF if self.byte else NAN)
        else:
            self.t.copy_(init)
        assert self.byte or self.t.data_ptr() % 16 == (4 if off16 else 0)

    def ptr(self):
        return self.t.data_ptr()

    def result(self, tag, finite=True):
        torch.cuda.synchronize()
        s = self.store.cpu()
        assert (s[:self.off] == self.fill).all() and (s[self.off + self.n:] == self.fill).all(), '%s: a guard beside the output was written' % tag
        got = s[self.off:self.off + self.n].view(self.t.shape).clone()
        if self.byte:
            assert (got <= 4).all(), '%s: index bytes left unwritten' % tag
        elif finite:
            assert torch.isfinite(got).all(), '%s: output elements left unwritten (NaN prefill) or not finite' % tag
        return got


def _in(t, off16=False):
    """A contiguous device copy of a CPU tensor (off16: a view 4 bytes into a larger allocation)."""
    t = t.contiguous().float()
    if not off16:
        d = t.to(DEV)
        assert d.data_ptr() % 16 == 0
        return d
    store = torch.empty(t.numel() + 4, device=DEV)
    v = store[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4
    return v


def _ws(nbytes):
    return torch.full((int(nbytes) // 4 + 16,), NAN, device=DEV), int(nbytes)


def _gather(lib, W, transpose, TA, TB, kh0=0, kw0=0, kstep=1, off16=False):
    """re2e_conv_weight_gather: (Cout,Cin,KH,KW) -> [r][a][b][c] at taps (kh0 + a kstep, kw0 + b kstep); transpose: r = ci, c = co."""
    Cout, Cin, KH, KW = W.shape
    shape = (Cin, TA, TB, Cout) if transpose else (Cout, TA, TB, Cin)
    store = torch.full((Cout * Cin * TA * TB + 4,), NAN, device=DEV)
    dst = store[1 if off16 else 0:][:Cout * Cin * TA * TB].view(shape)
    lib.call('re2e_conv_weight_gather', W.data_ptr(), dst.data_ptr(), Cout, Cin, KH, KW, int(transpose), TA, TB, kh0, kw0, kstep)
    return dst


def _once(lib, row, case, fam, plan, finite=True):
    """One run of the row's entry point on fresh buffers -> (result, index bytes or None), CPU tensors.  finite = False: the inputs hold NaN or
    infinities on purpose (tests/test_nonfinite_kernels_gpu.py), the caller checks where the output does."""
    N, H, W, Cin, Cout, k, s, pad = row.N, row.H, row.W, row.Cin, row.Cout, row.k, row.stride, row.pad
    OH, OW = case['OH'], case['OW']
    u = bool(row.flags & R.F_UNALIGNED)
    tag = R.case_id(row)
    ptr = lambda t: None if t is None else t.data_ptr()
    Wd = _in(case['w'], u)
    bias = _in(case['b'], u) if row.flags & R.F_BIAS else None
    idx = None
    if row.direction == R.FWD:
        x = _in(case['x'], u)
        pool = bool(row.flags & R.F_POOL)
        oshape = (N, (OH + 1) // 2, (OW + 1) // 2, Cout) if pool else (N, OH, OW, Cout)
        out = _Out(oshape, case['y0'] if row.beta else None, u)
        if pool:
            idx = _Out(oshape, dtype=torch.uint8)
        if fam == 'wino3x3':
            assert row.act in (R.ACT_NONE, R.ACT_RELU) and not row.beta
            ws, wsb = _ws(lib.query('re2e_conv3x3_wino_workspace_bytes', Cin, Cout))
            lib.call('re2e_conv3x3_wino', x.data_ptr(), N, H, W, Cin, Wd.data_ptr(), Cout, 0, ptr(bias), int(row.act == R.ACT_RELU), None,
                     None if pool else out.ptr(), out.ptr() if pool else None, idx.ptr() if pool else None, ws.data_ptr(), wsb)
        elif fam == 'wino4x4':
            assert row.act == R.ACT_NONE and bias is None and not pool and not row.beta
            ws, wsb = _ws(lib.query('re2e_conv4x4_wino_workspace_bytes', N, H, W, Cin, Cout, pad))
            lib.call('re2e_conv4x4_wino', x.data_ptr(), N, H, W, Cin, Wd.data_ptr(), Cout, pad, 0, out.ptr(), ws.data_ptr(), wsb)
        else:
            wg = _gather(lib, Wd, False, k, k, off16=u)
            if pool and plan['fused_pool'] == '1':
                lib.call('re2e_conv3x3_relu_pool', x.data_ptr(), N, H, W, Cin, wg.data_ptr(), Cout, ptr(bias), out.ptr(), idx.ptr())
            elif pool:
                full = _Out((N, OH, OW, Cout))
                lib.call('re2e_conv_igemm', x.data_ptr(), N, H, W, Cin, wg.data_ptr(), Cout, k, k, OH, OW, s, s, 1, 1, -pad, -pad, full.ptr(), OH, OW, 1, 1, 0, 0,
                         ptr(bias), row.act, 0.0)
                lib.call('re2e_maxpool2_fwd', full.ptr(), N, OH, OW, Cout, out.ptr(), idx.ptr(), 1)
                full.result(tag + ' (full resolution)', finite)
            else:
                lib.call('re2e_conv_igemm', x.data_ptr(), N, H, W, Cin, wg.data_ptr(), Cout, k, k, OH, OW, s, s, 1, 1, -pad, -pad, out.ptr(), OH, OW, 1, 1, 0, 0,
                         ptr(bias), row.act, float(row.beta))
    elif row.direction == R.DGRAD:
        dz = _in(case['dz'], u)
        mask = _in(case['x'], u) if row.flags & R.F_MASK else None
        # Cin == 1 at stride 2 and an odd size: one class is empty and its launch skipped, ops.conv_dgrad zero-fills there; not a case of these tables
        out = _Out((N, H, W, Cin), None, u)
        if fam == 'wino3x3':
            ws, wsb = _ws(lib.query('re2e_conv3x3_wino_workspace_bytes', Cout, Cin))
            lib.call('re2e_conv3x3_wino', dz.data_ptr(), N, H, W, Cout, Wd.data_ptr(), Cin, 1, None, 0, ptr(mask), out.ptr(), None, None, ws.data_ptr(), wsb)
        elif fam == 'wino4x4':
            assert mask is None
            ws, wsb = _ws(lib.query('re2e_conv4x4_wino_workspace_bytes', N, OH, OW, Cout, Cin, 3 - pad))
            lib.call('re2e_conv4x4_wino', dz.data_ptr(), N, OH, OW, Cout, Wd.data_ptr(), Cin, 3 - pad, 1, out.ptr(), ws.data_ptr(), wsb)
        elif s == 1:
            wt = _gather(lib, Wd, True, k, k, off16=u)
            if mask is not None:
                lib.call('re2e_conv_igemm_masked', dz.data_ptr(), N, OH, OW, Cout, wt.data_ptr(), Cin, k, k, H, W, 1, 1, -1, -1, pad, pad, out.ptr(), H, W, 1, 1, 0, 0,
                         mask.data_ptr())
            else:
                lib.call('re2e_conv_igemm', dz.data_ptr(), N, OH, OW, Cout, wt.data_ptr(), Cin, k, k, H, W, 1, 1, -1, -1, pad, pad, out.ptr(), H, W, 1, 1, 0, 0,
                         None, R.ACT_NONE, 0.0)
        elif Cin != 1:
            assert s == 2 and k % 2 == 0 and mask is None
            wt = torch.full((4 * Cin * (k // 2) * (k // 2) * Cout + 4,), NAN, device=DEV)
            lib.call('re2e_conv_dgrad_s2', dz.data_ptr(), N, OH, OW, Cout, Wd.data_ptr(), Cin, k, k, H, W, pad, out.ptr(), wt.data_ptr())
        else:      # the thin kernel: one launch per output parity class (ph, pw), taps a -> kh = 2 a + ((ph + pad) % 2)
            assert s == 2 and k % 2 == 0 and mask is None and H % 2 == 0 and W % 2 == 0
            T = k // 2
            for ph in range(2):
                for pw in range(2):
                    kh0, kw0 = (ph + pad) % 2, (pw + pad) % 2
                    wt = _gather(lib, Wd, True, T, T, kh0, kw0, 2, off16=u)
                    lib.call('re2e_conv_igemm', dz.data_ptr(), N, OH, OW, Cout, wt.data_ptr(), Cin, T, T, H // 2, W // 2, 1, 1, -1, -1, (ph + pad - kh0) // 2,
                             (pw + pad - kw0) // 2, out.ptr(), H, W, 2, 2, ph, pw, None, R.ACT_NONE, 0.0)
    else:
        x, dz = _in(case['x'], u), _in(case['dz'], u)
        out = _Out((Cout, Cin, k, k), case['dW0'] if row.beta else None, u)
        if fam == 'wino3x3':
            ws, wsb = _ws(lib.query('re2e_conv3x3_wino_wgrad_workspace_bytes', N, H, W, Cin, Cout))
            assert wsb == R.ww_workspace_bytes(N, H, W, Cin, Cout)
            lib.call('re2e_conv3x3_wino_wgrad', x.data_ptr(), N, H, W, Cin, dz.data_ptr(), Cout, out.ptr(), float(row.beta), ws.data_ptr(), wsb)
        elif fam == 'wino4x4':
            ws, wsb = _ws(lib.query('re2e_conv4x4_wino_wgrad_workspace_bytes', N, H, W, Cin, Cout, pad))
            assert wsb == R.w44_wgrad_sub(N, H, W, Cin, Cout, pad)[3]          # the K slices per position and the padded tile count the row declares
            lib.call('re2e_conv4x4_wino_wgrad', x.data_ptr(), N, H, W, Cin, dz.data_ptr(), Cout, pad, out.ptr(), float(row.beta), ws.data_ptr(), wsb)
        else:
            ws, wsb = _ws(lib.query('re2e_conv_wgrad_workspace_bytes', N, OH, OW, Cin, Cout, k, k))
            lib.call('re2e_conv_wgrad', x.data_ptr(), N, H, W, Cin, dz.data_ptr(), Cout, k, k, OH, OW, s, s, -pad, -pad, out.ptr(), float(row.beta), ws.data_ptr(), wsb)
    return out.result(tag, finite), None if idx is None else idx.result(tag + ' (index bytes)')


def _run(lib, row, case, fam, plan):
    """Twice on fresh buffers, on a filler stream where the row asks for one; the two results are equal bit for bit."""
    def both():
        return _once(lib, row, case, fam, plan), _once(lib, row, case, fam, plan)
    if row.flags & R.F_FILLER:
        st = torch.cuda.Stream()
        lib.set_stream_role(st, True)
        try:
            st.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(st):
                a, b = both()
            st.synchronize()
        finally:
            lib.set_stream_role(st, False)
    else:
        a, b = both()
    assert torch.equal(a[0], b[0]) and (a[1] is None or torch.equal(a[1], b[1])), '%s: two runs on fresh buffers differ' % R.case_id(row)
    return a


def _held(tag, q, fam, got, f64, yard):
    bar = R.BARS[q, fam]
    assert bar <= R.BAR_CAP
    cpu, err = R.rel_err(yard, f64), R.rel_err(got, f64)
    print('ERR %-78s %-4s %-7s hip %.2e  fp32-cpu %.2e  bar %.0e' % (tag, q, fam, err, cpu, bar))
    assert cpu <= bar / 8, 'input too hard for the bar: the fp32 CPU yardstick of %s is %.3e from float64, the bar is %.1e' % (tag, cpu, bar)
    assert err <= bar, '%s %s: HIP is %.3e of the max from float64 (bar %.1e, fp32 yardstick on the CPU: %.3e)' % (tag, q, err, bar, cpu)


def _check_index_bytes(tag, row, case, idx, vals64, idx64, bar):
    """The index bytes of a pooled forward: the float64 ones, except between window entries float64 itself holds closer than the bar (then any
    of them, and 4 -- nothing passes back -- only for a window whose maximum is within the bar of zero)."""
    if torch.equal(idx, idx64):
        return
    b = case['b'] if row.flags & R.F_BIAS else None
    y = R.conv_fwd(case['x'], case['w'], b, row.stride, row.pad, row.act)
    N, H, W, C = y.shape
    OH, OW = (H + 1) // 2, (W + 1) // 2
    win = torch.nn.functional.pad(y, (0, 0, 0, 2 * OW - W, 0, 2 * OH - H), value=float('-inf')).view(N, OH, 2, OW, 2, C).permute(0, 1, 3, 5, 2, 4).reshape(N, OH, OW, C, 4)
    tol = bar * y.abs().max().item()
    differ = idx != idx64
    picked = torch.where(idx >= 4, torch.zeros_like(vals64), win.gather(4, idx.clamp(max=3).long().unsqueeze(4)).squeeze(4))
    assert (vals64[differ] - picked[differ] <= tol).all(), '%s: %d index bytes name an entry that is not the maximum of its window' % (tag, int(differ.sum()))
    print('NOTE %s: %d of %d index bytes differ from float64 within near-ties' % (tag, int(differ.sum()), idx.numel()))


_DEVICE_ERROR = []          # the first device error of the session: nothing more is launched behind a fault


def _row_against_float64(row):
    if _DEVICE_ERROR:
        pytest.fail('not run: an earlier case ended in a device error (%s)' % _DEVICE_ERROR[0])
    ops, lib = _ops()
    try:
        _row_checked(ops, lib, row)
    except lib.Re2eError:
        raise
    except RuntimeError as e:          # torch's report of a HIP error: the device may be in no state to go on
        _DEVICE_ERROR.append('%s: %s' % (R.case_id(row), str(e).splitlines()[0]))
        raise


def _row_checked(ops, lib, row):
    args, flags = R.plan_args(row)
    plan = lib.conv_plan(*args, flags=flags)
    got_form = R.form_key(row.direction, plan)
    if row.form is not None:
        assert got_form == row.form, plan
        assert R.sub_of(row) == row.sub
    fam = R.family_of(row, plan['family'])
    case, r64, yard = _refs(_key(row), fam)
    out, idx = _run(lib, row, case, fam, plan)
    q = R.quantity_of(row)
    tag = '%s [%s]' % (R.case_id(row), '-'.join(str(v) for v in got_form))
    if row.flags & R.F_POOL:
        _held(tag, q, fam, out, r64[0], yard)
        _check_index_bytes(tag, row, case, idx, r64[0], r64[1], R.BARS[q, fam])
    else:
        _held(tag, q, fam, out, r64, yard)
    if row.flags & R.F_MASK:
        assert (out[case['x'] == 0] == 0).all() and (case['x'] == 0).any(), '%s: the gradient passes only where the ReLU output is > 0' % tag


@pytest.mark.parametrize('row', R.CONV_CASES, ids=R.case_id)
def test_convolution_forms_against_float64(row):
    _row_against_float64(row)


@pytest.mark.parametrize('row', R.EDGES, ids=R.case_id)
def test_convolution_edges_against_float64(row):
    _row_against_float64(row)


@pytest.mark.parametrize('layer', R.LAYERS, ids=R.layer_id)
def test_layers_against_float64(layer):
    """ops.conv2d / ops.conv_transpose2d and their autograd: y, dx, dW, db, each at the bar of the family its direction's plan names."""
    ops, lib = _ops()
    N, H, W, Cin, Cout, k, stride, act, bias, transposed = layer
    case = R.layer_case(layer)
    r64, r32 = R.layer_ref(layer, case), R.layer_ref(layer, case, torch.float32)
    x = case['x'].to(DEV).requires_grad_(True)
    w = torch.nn.Parameter(case['w'].to(DEV))
    b = torch.nn.Parameter(case['b'].to(DEV)) if bias else None
    if transposed:
        y = ops.conv_transpose2d(x, w, b, 2, 1)
        fams = ('direct',) * 3
    else:
        y = ops.conv2d(x, w, b, stride, 1, {R.ACT_NONE: None, R.ACT_RELU: 'relu', R.ACT_LRELU: 'lrelu'}[act])
        fams = tuple(lib.conv_plan(d, N, H, W, Cin, Cout, k, k, stride, 1, act=act if d == R.FWD else R.ACT_NONE, flags=R.F_BIAS if bias and d == R.FWD else 0)['family']
                     for d in (R.FWD, R.DGRAD, R.WGRAD))
    (y * case['go'].to(DEV)).sum().backward()
    torch.cuda.synchronize()
    got = dict(y=y.detach().cpu(), dx=x.grad.cpu(), dW=w.grad.cpu(), db=b.grad.cpu() if bias else None)
    for name, fam in (('y', fams[0]), ('dx', fams[1]), ('dW', fams[2]), ('db', 'direct')):
        if r64[name] is None:
            continue
        assert torch.isfinite(got[name]).all(), name
        bar = R.BARS[name, fam]
        cpu, err = R.rel_err(r32[name], r64[name]), R.rel_err(got[name], r64[name])
        print('ERR %-78s %-4s %-7s hip %.2e  fp32-cpu %.2e  bar %.0e' % (R.layer_id(layer), name, fam, err, cpu, bar))
        assert cpu <= bar / 8 and err <= bar, '%s %s: HIP is %.3e of the max from float64 (bar %.1e, fp32 on the CPU: %.3e)' % (R.layer_id(layer), name, err, bar, cpu)
