"""csrc/fbank.hip and the BatchNorm, pool / pack, loss-reduction and update kernels of csrc/elementwise.hip against the float64 references of
tests/refs64_feat.py, through the C ABI (lib.call), at the smallest shapes that reach each branch of their launchers (the tables of
refs64_feat; tests/test_refs64_feat_cpu.py checks what they cover, that every named mistake moves a case beyond its bar, and the
precondition of every bar: torch's fp32 CPU run of the same reference within a quarter of it).

Every call: outputs and workspaces are NaN before it (index bytes 0xFF), each output sits between guards inside one allocation, which
must come back untouched, and the call runs twice on fresh buffers: the second result must equal the first bit for bit.  The bars are
the project's own (test_kernels_gpu.py: test_fbank, test_bn_lrelu, test_mean_loss; re2e_sgd_step's 1e-6 for the norm and the update
state); the pool and the pack are exact.  Each quantity prints the HIP kernel's and the fp32 CPU run's distance from float64.  GPU only.

Measured on an MI355X when the module was written, worst case over the tables, HIP / fp32 on the CPU (of the tensor's max):
    filterbank: y_raw 1.1e-7 / 5.3e-8, y_norm 1.3e-7 / 1.0e-7, pw_out 2.4e-7 / 2.4e-7 (bar 1e-5); dx 1.7e-7 / 2.2e-7 (1e-4)
    dense tail: y 1.3e-7 / 1.1e-7 (1e-5), dz 8.4e-8 / 8.4e-8 (1e-4); CMVN sums 1.8e-7 / 1.2e-7, sums of squares 1.2e-7 / 1.1e-7 (1e-5)
    BatchNorm: y 3.2e-6 / 1.9e-6 (the case with mean 50, deviation 0.5; 2e-7 elsewhere), save_mean 2.3e-7 / 2.3e-7, save_invstd 1.5e-7 / 1.7e-7,
        running_mean 2.4e-7 / 2.1e-7, running_var 9.6e-8 / 1.0e-7 (1e-5); dx 2.6e-7 / 2.2e-7, dgamma 1.2e-5 / 6.2e-6 (P = 2), dbeta 3.3e-7 / 2.3e-7 (1e-4)
    BatchNorm over two ranks (3 : 5): every quantity 4e-8 .. 1.4e-7 / 4e-8 .. 1.8e-7
    losses: value 1.5e-7 / 1.4e-7, gradient 1.6e-7 / 1.5e-7 (1e-5); re2e_sumsq 4.7e-8 / 3.6e-8, clip stats 2e-11 / 2e-11 (1e-6)
    Adadelta: update of step 1 3.3e-7 / 2.5e-7 (bar 1e-6 = 4 x the fp32 CPU run's 2.5e-7); p of steps 2, 3 3.7e-7 / 2.9e-7, square_avg 3.3e-7 / 1.4e-7,
        acc_delta 5.6e-7 / 5.7e-7 (1e-6)
    Adam: update of step 1 2.8e-7 / 3.7e-7 (bar 2e-6 = 4 x 3.7e-7 rounded up); p of later steps 3.1e-7 / 3.2e-7, exp_avg 1.2e-7 / 1.2e-7,
        exp_avg_sq 2.4e-7 / 2.4e-7 (1e-6)
Before this module's fixes (float betas in re2e_adam_step's ABI, bias corrections by powf on the host; `v > best` from -3.0e38 in the three pools) the
same table gave Adam's exp_avg_sq 1.29e-5 and p of steps 2, 3 1.9e-6 .. 2.2e-6 against the 1e-6 bar (the update of step 1 passed at 3.3e-7: from a zero
state the float error of 1 - beta2 cancels against the float bias correction), and every NaN test of the pools failed: the stand-alone pool
returned the maximum of the other pixels (-3.0e38 for a window of -inf), the Winograd epilogue 0, the halo-patch epilogue the other pixels' maximum.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

import refs64_feat as R
from test_loss_kernels_gpu import DEV, _held, _i32, _ops

pytestmark = pytest.mark.gpu

NAN = float('nan')
GUARD = 64                       # floats (or bytes) on either side of an output
WORST = {}                       # quantity -> (worst HIP distance, worst fp32 CPU distance) over what has run


class _Out(object):
    """A device output between two guards inside one allocation, NaN (bytes: 0xFF) before the call; ``off``: elements past a 16-byte
    boundary the output starts at (floats: 1 = 4 bytes off; bytes: 1 = 1 byte off a 4-byte boundary)."""

    def __init__(self, shape, init=None, off=0, dtype=torch.float32):
        n = 1
        for v in shape:
            n *= v
        self.byte = dtype == torch.uint8
        self.n, self.start = n, GUARD + off
        self.store = torch.full((n + 2 * GUARD + 8,), 0xAB if self.byte else NAN, dtype=dtype, device=DEV)
        self.t = self.store[self.start:self.start + n].view(shape)
        if self.byte:
            self.t.fill_(0xFF)
        elif init is not None:
            self.t.copy_(init)
        assert self.t.data_ptr() % (4 if self.byte else 16) == (off if self.byte else 4 * off)

    def ptr(self):
        return self.t.data_ptr()

    def result(self, tag):
        torch.cuda.synchronize()
        s = self.store.cpu()
        lo, hi = s[:self.start], s[self.start + self.n:]
        ok = ((lo == 0xAB).all() and (hi == 0xAB).all()) if self.byte else (torch.isnan(lo).all() and torch.isnan(hi).all())
        assert ok, '%s: a guard beside the output was written' % tag
        return s[self.start:self.start + self.n].view(self.t.shape).clone()


def _in(t, off=0):
    """A contiguous device copy of a CPU tensor, ``off`` floats past a 16-byte boundary."""
    t = t.contiguous().float()
    store = torch.empty(t.numel() + 4, device=DEV)
    v = store[off:off + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 * off
    return v


def _ws(nbytes):
    return torch.full((int(nbytes) // 4 + GUARD,), NAN, device=DEV), int(nbytes)


def _ws_ok(ws, wsb, tag):
    assert torch.isnan(ws[wsb // 4:]).all(), '%s: written beyond the workspace it asked for' % tag


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def _same(a, b, tag):
    for k in a:
        assert (a[k] is None and b[k] is None) or torch.equal(_bits(a[k]), _bits(b[k])), '%s %s: the second run differs from the first' % (tag, k)


def _twice(run, tag):
    first, second = run(), run()
    _same(first, second, tag)
    return first


def _note(q, got, f64, f32):
    hip, cpu = R.rel_err(got, f64), R.rel_err(f32, f64)
    w = WORST.get(q, (0.0, 0.0))
    WORST[q] = (max(w[0], hip), max(w[1], cpu))
    return hip, cpu


def _check(case, q, got, f64, f32, bar, key=None):
    """_held (precondition, both distances printed, the bar asserted), and the worst distances kept for the summary."""
    assert torch.isfinite(got[torch.isfinite(f64)]).all(), '%s %s: not finite where the reference is' % (case, q)
    _note(key or q, got, f64, f32)
    _held(case, q, got, f64, f32, bar)


def _quiet(case, q, got, f64, f32, bar, key=None):
    """_check without the line (the combinations of optional operands repeat a quantity many times)."""
    assert torch.isfinite(got).all(), '%s %s: not finite where the reference is' % (case, q)
    hip, cpu = _note(key or q, got, f64, f32)
    assert cpu <= 0.25 * bar and hip <= bar, '%s %s: HIP is %.3e of the max from float64 (bar %.1e, fp32 on the CPU: %.3e)' % (case, q, hip, bar, cpu)


# ---------------------------------------------------------------------------------------------
# filterbank
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _fbank_refs(bank, rows):
    case = R.fbank_case((bank, rows, None))
    return case, {ins: (R.fbank_case_ref(case, ins), R.fbank_case_ref(case, ins, torch.float32)) for ins in R.FBANK_BWD_INS}


@pytest.mark.parametrize('row', R.FBANK_CASES, ids=R.fbank_case_id)
def test_fbank_against_float64(row):
    ops, lib = _ops()
    bank, rows, mis = row
    tag = R.fbank_case_id(row)
    case, refs = _fbank_refs(bank, rows)
    Fd, NF = case['F'], case['NF']
    b = R.band_tables(case['W'])
    assert b['maxw'] <= 32 and b['maxc'] <= 128
    x = _in(case['x'])
    boff, blen, taps = _i32(b['off']), _i32(b['len']), _in(torch.from_numpy(b['taps']))
    toff, tlen, tw = _i32(b['toff']), _i32(b['tlen']), _in(torch.from_numpy(b['tw']))
    cm = _in(case['cmvn'], 1 if mis == 'cmvn' else 0)
    p = lambda o: None if o is None else o.ptr()
    r64, r32 = refs[(True, True)]
    dead, uncovered = torch.from_numpy(b['len'] == 0), torch.from_numpy(b['tlen'] == 0)
    pw_dev = None
    for outs in R.FBANK_FWD_OUTS:
        def run():
            o = [_Out((rows, NF)) if present else None for present in outs]
            lib.call('re2e_fbank_fwd', x.data_ptr(), rows, Fd, NF, boff.data_ptr(), blen.data_ptr(), taps.data_ptr(), b['maxw'], p(o[0]), p(o[1]),
                     cm.data_ptr() if outs[1] else None, p(o[2]))
            return {k: (v.result('%s %s' % (tag, k)) if v is not None else None) for k, v in zip(('y_raw', 'y_norm', 'pw'), o)}
        got = _twice(run, tag)
        full = outs == (True, True, True)
        for k in ('y_raw', 'y_norm', 'pw'):
            if got[k] is not None:
                (_check if full else _quiet)(tag, k, got[k], r64[k], r32[k], R.BAR_FBANK_OUT, 'fbank ' + k)
        if got['y_raw'] is not None and dead.any():
            assert (got['y_raw'][:, dead] == got['y_raw'][0, dead][0]).all(), 'an all-zero filter is log(1e-7) in every frame'
        if got['pw'] is not None:
            assert (got['pw'][:, dead] == 0).all()
            pw_dev = got['pw']
    for ins in R.FBANK_BWD_INS:
        r64, r32 = refs[ins]
        pw = _in(pw_dev, 1 if mis == 'pw' else 0)
        dyr = _in(case['g_raw'], 1 if mis == 'dy_raw' else 0) if ins[0] else None
        dyn = _in(case['g_norm'], 1 if mis == 'dy_norm' else 0) if ins[1] else None

        def run():
            dx = _Out((rows, Fd))
            lib.call('re2e_fbank_bwd', x.data_ptr(), rows, Fd, NF, toff.data_ptr(), tlen.data_ptr(), tw.data_ptr(), b['maxc'], pw.data_ptr(),
                     None if dyr is None else dyr.data_ptr(), None if dyn is None else dyn.data_ptr(), cm.data_ptr() if ins[1] else None, dx.ptr())
            return dict(dx=dx.result(tag + ' dx'))
        got = _twice(run, tag)
        (_check if ins == (True, True) else _quiet)(tag, 'dx', got['dx'], r64['dx'], r32['dx'], R.BAR_FBANK_GRAD, 'fbank dx')
        assert (got['dx'][:, uncovered] == 0).all(), 'a bin no filter covers has an exactly zero gradient'
        if rows >= 33:
            assert (got['dx'][:3] == 0).all(), 'frames on which the clamp fired pass no gradient'


@pytest.mark.parametrize('rows,N,with_cmvn', R.LOGCLAMP_CASES)
def test_logclamp_against_float64(rows, N, with_cmvn):
    ops, lib = _ops()
    tag = 'logclamp-%dx%d%s' % (rows, N, '-cmvn' if with_cmvn else '')
    c = R.logclamp_case(rows, N)
    cm = c['cmvn'] if with_cmvn else None
    r64, r32 = R.logclamp_ref(c['z'], cm, c['dy']), R.logclamp_ref(c['z'], cm, c['dy'], torch.float32)
    z, dy, cmd = _in(c['z']), _in(c['dy']), _in(c['cmvn']) if with_cmvn else None

    def run():
        y, dz = _Out((rows, N)), _Out((rows, N))
        lib.call('re2e_logclamp_fwd', z.data_ptr(), None if cmd is None else cmd.data_ptr(), rows, N, y.ptr())
        lib.call('re2e_logclamp_bwd', z.data_ptr(), None if cmd is None else cmd.data_ptr(), rows, N, dy.data_ptr(), dz.ptr())
        return dict(y=y.result(tag + ' y'), dz=dz.result(tag + ' dz'))
    got = _twice(run, tag)
    _check(tag, 'y', got['y'], r64['y'], r32['y'], R.BAR_FBANK_OUT, 'logclamp y')
    _check(tag, 'dz', got['dz'], r64['dz'], r32['dz'], R.BAR_FBANK_GRAD, 'logclamp dz')
    assert (got['dz'][c['z'] <= 1e-8] == 0).all(), 'the clamp passes no gradient'


@pytest.mark.parametrize('B,T,NF,lens', R.CMVN_CASES)
def test_cmvn_stats_against_float64(B, T, NF, lens):
    ops, lib = _ops()
    tag = 'cmvn-%dx%dx%d' % (B, T, NF)
    y = R.cmvn_case(B, T, NF)
    yd, ld = _in(y), _i32(lens)

    def run():
        s, q = _Out((NF,)), _Out((NF,))
        lib.call('re2e_cmvn_stats', yd.data_ptr(), ld.data_ptr(), B, T, NF, s.ptr(), q.ptr())
        return dict(sum=s.result(tag + ' sum'), sumsq=q.result(tag + ' sumsq'))
    got = _twice(run, tag)
    for k, a, b in zip(('sum', 'sumsq'), R.cmvn_stats_ref(y, lens), R.cmvn_stats_ref(y, lens, torch.float32)):
        _check(tag, k, got[k], a, b, R.BAR_FBANK_OUT, 'cmvn ' + k)


# ---------------------------------------------------------------------------------------------
# BatchNorm + LeakyReLU
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _bn_refs(row):
    c = R.bn_case(row[0], row[1], row[5], row[2])
    return c, R.bn_case_ref(row, c), R.bn_case_ref(row, c, torch.float32)


def _bn_forward(lib, c, P, C, train, slope, x, tag):
    ga, be = _in(c['gamma']), _in(c['beta'])
    wsb = lib.query('re2e_bn_workspace_bytes', P, C)

    def run():
        rm, rv = _Out((C,), c['rm']), _Out((C,), c['rv'])
        y, sm, si = _Out((P, C)), _Out((C,)), _Out((C,))
        ws, _ = _ws(wsb)
        lib.call('re2e_bn_lrelu_fwd', x.data_ptr(), P, C, ga.data_ptr(), be.data_ptr(), rm.ptr(), rv.ptr(), R.BN_MOMENTUM, R.BN_EPS, int(train), slope,
                 y.ptr(), sm.ptr(), si.ptr(), ws.data_ptr(), wsb)
        out = dict(y=y.result(tag + ' y'), save_mean=sm.result(tag + ' save_mean'), save_invstd=si.result(tag + ' save_invstd'),
                   running_mean=rm.result(tag + ' running_mean'), running_var=rv.result(tag + ' running_var'))
        _ws_ok(ws, wsb, tag)
        return out
    return _twice(run, tag), ga, be, wsb


@pytest.mark.parametrize('row', R.BN_CASES, ids=R.bn_case_id)
def test_bn_lrelu_against_float64(row):
    ops, lib = _ops()
    P, C, slope, gbeta, train, special = row
    tag = R.bn_case_id(row)
    c, r64, r32 = _bn_refs(row)
    x = _in(c['x'], 1 if special == 'x-misaligned' else 0)
    got, ga, be, wsb = _bn_forward(lib, c, P, C, train, slope, x, tag)
    for k in ('y', 'save_mean', 'save_invstd', 'running_mean', 'running_var'):
        _check(tag, k, got[k], r64[k], r32[k], R.BAR_BN_OUT, 'bn ' + k)
    if not train:
        assert torch.equal(got['running_mean'], c['rm']) and torch.equal(got['running_var'], c['rv']), 'eval mode leaves the running statistics alone'
        assert torch.equal(got['save_mean'], c['rm'])
        return
    dy, sm, si = _in(c['dy']), _in(got['save_mean']), _in(got['save_invstd'])

    def run():
        dx = _Out((P, C))
        dg, db = (_Out((C,), None if gbeta == 0.0 else c[k]) for k in ('dgamma0', 'dbeta0'))
        ws, _ = _ws(wsb)
        lib.call('re2e_bn_lrelu_bwd', dy.data_ptr(), x.data_ptr(), P, C, ga.data_ptr(), be.data_ptr(), sm.data_ptr(), si.data_ptr(), slope, dx.ptr(),
                 dg.ptr(), db.ptr(), gbeta, ws.data_ptr(), wsb)
        out = dict(dx=dx.result(tag + ' dx'), dgamma=dg.result(tag + ' dgamma'), dbeta=db.result(tag + ' dbeta'))
        _ws_ok(ws, wsb, tag)
        return out
    back = _twice(run, tag)
    keep = ~R.bn_flip_band(r64['y'])
    assert float((~keep).float().mean()) <= 1e-3
    _check(tag, 'dx', back['dx'][keep], r64['dx'][keep], r32['dx'][keep], R.BAR_BN_GRAD, 'bn dx')
    assert torch.isfinite(back['dx']).all()
    _check(tag, 'dgamma', back['dgamma'], r64['dgamma'], r32['dgamma'], R.BAR_BN_GRAD, 'bn dgamma')
    _check(tag, 'dbeta', back['dbeta'], r64['dbeta'], r32['dbeta'], R.BAR_BN_GRAD, 'bn dbeta')


def test_bn_batch_with_a_nan_leaves_the_running_statistics_alone():
    """bn_finalize_kernel's documented departure from torch: a channel whose batch statistics are not finite keeps its running statistics
    bit for bit (the trainer repeats such a step); the other channels are updated as ever, and the NaN reaches y."""
    ops, lib = _ops()
    P, C = 255, 4
    row = (P, C, 0.2, 0.0, True, None)
    c = dict(_bn_refs(row)[0])
    c['x'] = c['x'].clone()
    c['x'][5, 1] = NAN
    got, _, _, _ = _bn_forward(lib, c, P, C, True, 0.2, _in(c['x']), 'bn-nan')
    assert got['running_mean'][1] == c['rm'][1] and got['running_var'][1] == c['rv'][1]
    assert torch.isnan(got['y'][:, 1]).all() and torch.isnan(got['save_mean'][1])
    ok = [0, 2, 3]
    r64 = R.bn_case_ref(row, c)
    for k in ('y', 'running_mean', 'running_var'):
        assert R.rel_err(got[k][..., ok], r64[k][..., ok]) <= R.BAR_BN_OUT, k


def test_bn_sync_path_against_float64_of_the_whole_batch():
    """Two "ranks" hold 3/8 and 5/8 of the rows: re2e_bn_sync_partial -> host sum -> re2e_bn_sync_finalize -> re2e_bn_apply ->
    re2e_bn_sync_bwd_partial -> host sum scaled by P / Ptotal -> re2e_bn_sync_bwd_apply, against the reference of the whole batch."""
    ops, lib = _ops()
    Pt, C, slope = R.BN_SYNC_CASE
    row = (Pt, C, slope, 0.0, True, None)
    c = R.bn_case(Pt, C, None, slope)
    r64, r32 = R.bn_case_ref(row, c), R.bn_case_ref(row, c, torch.float32)
    cut = Pt * 3 // 8
    parts = [(0, cut), (cut, Pt)]
    ga, be = _in(c['gamma']), _in(c['beta'])
    xs = [_in(c['x'][a:b]) for a, b in parts]
    dys = [_in(c['dy'][a:b]) for a, b in parts]

    def partial(x, P, mean, square):
        wsb = lib.query('re2e_bn_workspace_bytes', P, C)
        ws, _ = _ws(wsb)
        out = _Out((C,))
        lib.call('re2e_bn_sync_partial', x.data_ptr(), P, C, None if mean is None else mean.data_ptr(), square, out.ptr(), ws.data_ptr(), wsb)
        r = out.result('sync partial')
        _ws_ok(ws, wsb, 'sync partial')
        return r

    def run():
        mean = _in(sum(partial(x, b - a, None, 0) for x, (a, b) in zip(xs, parts)) / float(Pt))
        var = _in(sum(partial(x, b - a, mean, 1) for x, (a, b) in zip(xs, parts)) / float(Pt))
        rm, rv, sm, si = _Out((C,), c['rm']), _Out((C,), c['rv']), _Out((C,)), _Out((C,))
        lib.call('re2e_bn_sync_finalize', mean.data_ptr(), var.data_ptr(), Pt, C, R.BN_MOMENTUM, R.BN_EPS, rm.ptr(), rv.ptr(), sm.ptr(), si.ptr())
        out = dict(save_mean=sm.result('sync save_mean'), save_invstd=si.result('sync save_invstd'), running_mean=rm.result('sync running_mean'),
                   running_var=rv.result('sync running_var'))
        ys, sums = [], []
        for x, dy, (a, b) in zip(xs, dys, parts):
            y = _Out((b - a, C))
            lib.call('re2e_bn_apply', x.data_ptr(), b - a, C, sm.ptr(), si.ptr(), ga.data_ptr(), be.data_ptr(), slope, y.ptr())
            ys.append(y.result('sync y'))
            wsb = lib.query('re2e_bn_workspace_bytes', b - a, C)
            ws, _ = _ws(wsb)
            s = _Out((2 * C,))
            lib.call('re2e_bn_sync_bwd_partial', dy.data_ptr(), x.data_ptr(), b - a, C, ga.data_ptr(), be.data_ptr(), sm.ptr(), si.ptr(), slope, s.ptr(),
                     ws.data_ptr(), wsb)
            sums.append(s.result('sync sums'))
            _ws_ok(ws, wsb, 'sync bwd partial')
        tot = sums[0] + sums[1]
        dxs = []
        for x, dy, (a, b) in zip(xs, dys, parts):
            dx = _Out((b - a, C))
            scaled = _in(tot * (float(b - a) / float(Pt)))
            lib.call('re2e_bn_sync_bwd_apply', dy.data_ptr(), x.data_ptr(), b - a, C, ga.data_ptr(), be.data_ptr(), sm.ptr(), si.ptr(), slope,
                     scaled.data_ptr(), dx.ptr())
            dxs.append(dx.result('sync dx'))
        out.update(y=torch.cat(ys), dx=torch.cat(dxs), dgamma=tot[C:].clone(), dbeta=tot[:C].clone())
        return out
    got = _twice(run, 'bn-sync')
    assert not R.bn_flip_band(r64['y']).any()
    for k, bar in R.BN_QUANTITIES:
        _check('bn-sync-3:5', k, got[k], r64[k], r32[k], bar, 'bn-sync ' + k)


# ---------------------------------------------------------------------------------------------
# pool and pack: exact
# ---------------------------------------------------------------------------------------------
def _pool_hip(lib, x, relu_in, idx_off, tag):
    NI, H, W, C = x.shape
    OH, OW = (H + 1) // 2, (W + 1) // 2
    xd = _in(x)

    def run():
        out, idx = _Out((NI, OH, OW, C)), _Out((NI, OH, OW, C), off=idx_off, dtype=torch.uint8)
        lib.call('re2e_maxpool2_fwd', xd.data_ptr(), NI, H, W, C, out.ptr(), idx.ptr(), int(relu_in))
        return dict(out=out.result(tag + ' out'), idx=idx.result(tag + ' idx'))
    return _twice(run, tag)


def _equal_with_nans(got, want, tag):
    assert torch.equal(torch.isnan(got), torch.isnan(want)), '%s: the NaN patterns differ' % tag
    fin = ~torch.isnan(want)
    assert torch.equal(got[fin], want[fin]), '%s: values differ' % tag


@pytest.mark.parametrize('relu_in', [0, 1])
@pytest.mark.parametrize('NI,H,W,C,idx_off', R.POOL_CASES)
def test_maxpool_exact(NI, H, W, C, idx_off, relu_in):
    ops, lib = _ops()
    tag = 'pool-%dx%dx%dx%d-relu%d' % (NI, H, W, C, relu_in)
    x = R.pool_case(NI, H, W, C)
    want, widx = R.pool_ref(x, bool(relu_in))
    got = _pool_hip(lib, x, relu_in, int(idx_off), tag)
    assert torch.equal(got['out'], want) and torch.equal(got['idx'], widx)
    if relu_in:
        assert (got['idx'][0, 0, 0] == 4).all()
    g = torch.Generator().manual_seed(NI + H)
    dout = R.rnd(g, *want.shape)
    dd = _in(dout)
    ib = _Out(want.shape, off=int(idx_off), dtype=torch.uint8)
    ib.t.copy_(widx)

    def run():
        din = _Out((NI, H, W, C))
        lib.call('re2e_maxpool2_bwd', dd.data_ptr(), ib.ptr(), NI, H, W, C, din.ptr())
        return dict(din=din.result(tag + ' din'))
    assert torch.equal(_twice(run, tag)['din'], R.pool_bwd_ref(dout, widx, H, W))


@pytest.mark.parametrize('relu_in', [0, 1])
@pytest.mark.parametrize('C', [6, 8])
def test_maxpool_propagates_nan_like_torch(C, relu_in):
    """A window holding a NaN pools to NaN (torch.max_pool2d; the NaN gate of the joint step must see it whichever pool ran), a window of
    -inf pools to -inf, +inf stays +inf; the index byte is torch's (the last NaN), 4 under relu_in."""
    ops, lib = _ops()
    x = R.pool_nan_case(3, 37, 21, C)
    want, widx = R.pool_ref(x, bool(relu_in))
    assert torch.isnan(want).sum() >= 4 and (want == -R.INF).any()
    got = _pool_hip(lib, x, relu_in, 0, 'pool-nan-C%d-relu%d' % (C, relu_in))
    _equal_with_nans(got['out'], want, 'pool')
    assert torch.equal(got['idx'], widx)


@pytest.mark.parametrize('NI,T,Fq,C,NItot,noff,lens', R.PACK_CASES)
def test_vgg_pack_exact(NI, T, Fq, C, NItot, noff, lens):
    ops, lib = _ops()
    tag = 'pack-%dx%dx%dx%d' % (NI, T, Fq, C)
    g = torch.Generator().manual_seed(T * Fq + C)
    src, dout = R.rnd(g, NI, T, Fq, C), R.rnd(g, T, NItot, C * Fq)
    sd, dd, ld = _in(src), _in(dout), _i32(lens)

    def run():
        out, din = _Out((T, NItot, C * Fq)), _Out((NI, T, Fq, C))
        lib.call('re2e_vgg_pack_fwd', sd.data_ptr(), ld.data_ptr(), NI, T, Fq, C, out.ptr(), NItot, noff)
        lib.call('re2e_vgg_pack_bwd', dd.data_ptr(), ld.data_ptr(), NI, T, Fq, C, din.ptr(), NItot, noff)
        return dict(out=out.result(tag + ' out'), din=din.result(tag + ' din'))
    got = _twice(run, tag)
    _equal_with_nans(got['out'], R.pack_ref(src, lens, NItot, noff, torch.full((T, NItot, C * Fq), NAN)), tag + ' (rows of another branch stay untouched)')
    assert torch.equal(got['din'], R.pack_bwd_ref(dout, lens, NI, noff, Fq, C))


def _fused_pool_case(N, H, W, Cin, Cout):
    """Inputs of test_conv_relu_pool_one_launch with one NaN in x -> x, weight, bias, torch's pooled result, pooled windows near the NaN."""
    g = torch.Generator().manual_seed(H + W)
    x, Wt, b = R.rnd(g, N, H, W, Cin), R.rnd(g, Cout, Cin, 3, 3, scale=0.15), R.rnd(g, Cout, scale=0.3)
    py, px = 5, 3
    x[N - 1, py, px, 1] = NAN
    ref = F.max_pool2d(F.relu(F.conv2d(x.permute(0, 3, 1, 2), Wt, b, padding=1)), 2, stride=2, ceil_mode=True).permute(0, 2, 3, 1)
    near = torch.zeros(1, 1, H, W)
    near[0, 0, max(py - 3, 0):py + 4, max(px - 3, 0):px + 4] = 1.0
    near = F.max_pool2d(near, 2, stride=2, ceil_mode=True)[0, 0] > 0
    far = torch.ones(N, *near.shape, dtype=torch.bool)
    far[N - 1] = ~near
    return x, Wt, b, ref, far


def _fused_pool_checks(tag, fused, unfused, ref, far):
    """The fused epilogue against conv -> ReLU -> re2e_maxpool2_fwd(relu_in) bit for bit, and against torch by the rule of
    test_conv_relu_propagates_nan_like_torch: every pooled output that is NaN in torch is NaN, outputs more than 3 pixels away are the
    finite reference values."""
    assert torch.isnan(ref).any() and torch.isfinite(ref[far]).all()
    _equal_with_nans(fused['out'], unfused['out'], tag + ': fused against conv -> pool')
    assert torch.equal(fused['idx'], unfused['idx']), '%s: index bytes of the fused and the stand-alone pool differ' % tag
    for what, got in (('fused', fused), ('conv -> pool', unfused)):
        assert torch.isnan(got['out'])[torch.isnan(ref)].all(), '%s (%s): a NaN of torch\'s max_pool2d(relu(conv2d)) was dropped' % (tag, what)
        assert torch.isfinite(got['out'][far]).all()
        assert (got['out'][far] - ref[far]).abs().max() <= 2e-4 * ref[far].abs().max()
        assert (got['idx'][torch.isnan(got['out'])] == 4).all()


@pytest.mark.parametrize('N,H,W,Cin,Cout', [(2, 37, 19, 16, 64), (1, 40, 83, 64, 64), (2, 33, 8, 128, 128)])
def test_winograd_pool_epilogue_propagates_nan(N, H, W, Cin, Cout):
    ops, lib = _ops()
    tag = 'wino-pool-nan-%dx%dx%dx%d-%d' % (N, H, W, Cin, Cout)
    assert lib.conv_plan(lib.CONV_FWD, N, H, W, Cin, Cout, 3, 3, 1, 1, act=lib.ACT_RELU, flags=lib.CONV_BIAS | lib.CONV_POOL)['family'] == 'wino3x3'
    x, Wt, b, ref, far = _fused_pool_case(N, H, W, Cin, Cout)
    xd, Wd, bd = _in(x), _in(Wt), _in(b)
    wsb = lib.query('re2e_conv3x3_wino_workspace_bytes', Cin, Cout)
    OH, OW = (H + 1) // 2, (W + 1) // 2

    def run(pool):
        def go():
            ws, _ = _ws(wsb)
            out, idx = _Out((N, OH, OW, Cout)), _Out((N, OH, OW, Cout), dtype=torch.uint8)
            if pool:
                lib.call('re2e_conv3x3_wino', xd.data_ptr(), N, H, W, Cin, Wd.data_ptr(), Cout, 0, bd.data_ptr(), 1, None, None, out.ptr(), idx.ptr(),
                         ws.data_ptr(), wsb)
            else:
                y = _Out((N, H, W, Cout))
                lib.call('re2e_conv3x3_wino', xd.data_ptr(), N, H, W, Cin, Wd.data_ptr(), Cout, 0, bd.data_ptr(), 1, None, y.ptr(), None, None,
                         ws.data_ptr(), wsb)
                lib.call('re2e_maxpool2_fwd', y.ptr(), N, H, W, Cout, out.ptr(), idx.ptr(), 1)
                y.result(tag + ' y')
            return dict(out=out.result(tag + ' out'), idx=idx.result(tag + ' idx'))
        return go
    _fused_pool_checks(tag, _twice(run(True), tag), _twice(run(False), tag), ref, far)


@pytest.mark.parametrize('N,H,W,Cin,Cout', [(2, 37, 19, 16, 64), (2, 33, 8, 128, 128)])
def test_halo_pool_epilogue_propagates_nan(N, H, W, Cin, Cout):
    ops, lib = _ops()
    tag = 'halo-pool-nan-%dx%dx%dx%d-%d' % (N, H, W, Cin, Cout)
    x, Wt, b, ref, far = _fused_pool_case(N, H, W, Cin, Cout)
    xd, bd = _in(x), _in(b)
    wg = torch.empty(Cout, 3, 3, Cin, device=DEV)
    lib.call('re2e_conv_weight_gather', _in(Wt).data_ptr(), wg.data_ptr(), Cout, Cin, 3, 3, 0, 3, 3, 0, 0, 1)
    OH, OW = (H + 1) // 2, (W + 1) // 2

    def run(pool):
        def go():
            out, idx = _Out((N, OH, OW, Cout)), _Out((N, OH, OW, Cout), dtype=torch.uint8)
            if pool:
                lib.call('re2e_conv3x3_relu_pool', xd.data_ptr(), N, H, W, Cin, wg.data_ptr(), Cout, bd.data_ptr(), out.ptr(), idx.ptr())
            else:
                y = _Out((N, H, W, Cout))
                lib.call('re2e_conv_igemm', xd.data_ptr(), N, H, W, Cin, wg.data_ptr(), Cout, 3, 3, H, W, 1, 1, 1, 1, -1, -1, y.ptr(), H, W, 1, 1, 0, 0,
                         bd.data_ptr(), lib.ACT_RELU, 0.0)
                lib.call('re2e_maxpool2_fwd', y.ptr(), N, H, W, Cout, out.ptr(), idx.ptr(), 1)
                y.result(tag + ' y')
            return dict(out=out.result(tag + ' out'), idx=idx.result(tag + ' idx'))
        return go
    _fused_pool_checks(tag, _twice(run(True), tag), _twice(run(False), tag), ref, far)


# ---------------------------------------------------------------------------------------------
# loss reductions
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _loss_refs(row):
    c = R.loss_case(row)
    return c, R.loss_case_ref(row, c), R.loss_case_ref(row, c, torch.float32)


@pytest.mark.parametrize('row', R.LOSS_CASES, ids=R.loss_case_id)
def test_loss_against_float64(row):
    ops, lib = _ops()
    kind, n, tk, gs, beta = row
    tag = R.loss_case_id(row)
    c, (v64, d64), (v32, d32) = _loss_refs(row)
    a = _in(c['a'])
    tensor_target = isinstance(c['t'], torch.Tensor)
    bt = _in(c['t']) if tensor_target else None
    target = 0.0 if tensor_target else float(c['t'])
    gsc = torch.tensor([R.LOSS_GSCALE], device=DEV) if gs else None
    wsb = lib.query('re2e_reduce_workspace_bytes', n)

    def run():
        ws, _ = _ws(wsb)
        out = _Out((1,))
        lib.call('re2e_loss_fwd', a.data_ptr(), None if bt is None else bt.data_ptr(), target, n, kind, out.ptr(), ws.data_ptr(), wsb)
        da = _Out((n,), None if beta == 0.0 else c['da0'])
        lib.call('re2e_loss_bwd', a.data_ptr(), None if bt is None else bt.data_ptr(), target, n, kind, None if gsc is None else gsc.data_ptr(),
                 R.LOSS_SCALE, da.ptr(), beta)
        r = dict(value=out.result(tag + ' value'), da=da.result(tag + ' da'))
        _ws_ok(ws, wsb, tag)
        return r
    got = _twice(run, tag)
    _check(tag, 'value', got['value'].view(()), v64, v32, R.BAR_LOSS, 'loss value')
    _check(tag, 'da', got['da'], d64, d32, R.BAR_LOSS, 'loss gradient')
    if kind in (R.L1, R.SMOOTH_L1) and beta == 0.0:
        d = c['a'] - c['t']
        assert (got['da'][d == 0] == 0).all(), 'd = 0: an exactly zero gradient'


# ---------------------------------------------------------------------------------------------
# gradient norm, clip coefficient, updates
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _grads():
    return R.update_grads()


@pytest.mark.parametrize('n,misaligned', R.SUMSQ_CASES)
def test_sumsq_against_float64(n, misaligned):
    ops, lib = _ops()
    tag = 'sumsq-n%d%s' % (n, '-misaligned' if misaligned else '')
    x = _grads()[0][0][:n]
    xd = _in(x, 1 if misaligned else 0)
    wsb = lib.query('re2e_reduce_workspace_bytes', n)

    def run():
        ws, _ = _ws(wsb)
        out = _Out((1,))
        lib.call('re2e_sumsq', xd.data_ptr(), n, out.ptr(), ws.data_ptr(), wsb)
        r = dict(sumsq=out.result(tag))
        _ws_ok(ws, wsb, tag)
        return r
    got = _twice(run, tag)
    _check(tag, 'sumsq', got['sumsq'].view(()), R.sumsq_ref(x), R.sumsq_ref(x, torch.float32), R.BAR_SUM, 'sumsq')


@pytest.mark.parametrize('sumsq,max_norm', R.CLIP_CASES)
def test_clip_coef_against_float64(sumsq, max_norm):
    ops, lib = _ops()
    tag = 'clip-%g' % sumsq
    s = torch.tensor([sumsq], device=DEV)

    def run():
        st = _Out((6,))
        lib.call('re2e_clip_coef', s.data_ptr(), max_norm, st.ptr())
        return dict(stats=st.result(tag))
    got = _twice(run, tag)['stats']
    want = R.clip_ref(torch.tensor(sumsq), max_norm)
    if want[2] == 0:
        assert got[2] == 0 and got[5] == 0, 'an inf or NaN norm must close the gate in both triples'
        return
    _check(tag, 'stats', got, want, R.clip_ref(torch.tensor(sumsq), max_norm, torch.float32), R.BAR_SUM, 'clip stats')
    assert got[2] == 1 and got[5] == 1 and got[4] == 1 and got[3] == got[0] and (got[1] == 1) == (float(want[1]) == 1.0)


def _update_hip(lib, row, grads, state):
    """The steps of a row on the device from the carried state -> list of (p, s1, s2) CPU tensors after each step."""
    opt, betas, sk, start = row
    n = grads[0].numel()
    st = torch.tensor(R.UPDATE_STATS[sk], device=DEV) if R.UPDATE_STATS[sk] is not None else None
    if start == 'zero':
        init, steps = (torch.zeros(n),) * 3, (1, 2, 3)
    else:
        init, steps = (state['p'], state['m'], state['v']), (1000,)
    bufs = [_Out((n,), t) for t in init]
    out = []
    for k, step in enumerate(steps):
        g = _in(grads[k])
        if opt == 'adam':
            lib.call('re2e_adam_step', bufs[0].ptr(), g.data_ptr(), bufs[1].ptr(), bufs[2].ptr(), n, R.ADAM_HYPER['lr'], betas[0], betas[1], R.ADAM_HYPER['eps'],
                     step, None if st is None else st.data_ptr())
        else:
            lib.call('re2e_adadelta_step', bufs[0].ptr(), g.data_ptr(), bufs[1].ptr(), bufs[2].ptr(), n, R.ADADELTA_HYPER['rho'], R.ADADELTA_HYPER['eps'],
                     R.ADADELTA_HYPER['lr'], None if st is None else st.data_ptr())
        out.append(tuple(b.result('%s step %d' % (R.update_case_id(row), step)) for b in bufs))
    return out


@pytest.mark.parametrize('row', R.UPDATE_CASES, ids=R.update_case_id)
def test_update_steps_against_float64(row):
    """p and both state tensors after each step.  p after step 1 from p = 0 is the negated update, read without cancellation: its bar
    (refs64_feat.BAR_UPDATE) is 4 x the fp32 CPU run's own worst distance; everything else takes 1e-6 (refs64_feat.BAR_SUM).  Precondition:
    the fp32 CPU run within refs64_feat.UPDATE_MARGIN of the bar (see there)."""
    ops, lib = _ops()
    grads, state = _grads()
    tag = R.update_case_id(row)
    r64, r32 = R.update_run(row, grads, state), R.update_run(row, grads, state, torch.float32)
    first, second = _update_hip(lib, row, grads, state), _update_hip(lib, row, grads, state)
    names = ('p', 'exp_avg', 'exp_avg_sq') if row[0] == 'adam' else ('p', 'square_avg', 'acc_delta')
    bad = []
    for k in range(len(r64)):
        for q in range(3):
            assert torch.equal(_bits(first[k][q]), _bits(second[k][q])), '%s: the second run differs from the first' % tag
            assert torch.isfinite(first[k][q]).all()
            bar, step = R.update_bar(row, k, q), 1000 if row[3] == 'step1000' else k + 1
            what = 'update step 1' if R.is_first_update(row, k, q) else names[q] if q else 'p, later steps'
            hip, cpu = _note('%s %s' % (row[0], what), first[k][q], r64[k][q], r32[k][q])
            print('ERR %-46s %-16s hip %.2e  fp32-cpu %.2e  bar %.0e' % (tag, '%s step %d' % (names[q], step), hip, cpu, bar))
            assert cpu <= R.UPDATE_MARGIN * bar, 'input too hard for the bar'
            if not hip <= bar:
                bad.append(('%s step %d' % (names[q], step), hip, bar))
    assert not bad, bad


@pytest.mark.parametrize('opt', ['adam', 'adadelta'])
def test_update_is_skipped_bit_for_bit_when_the_gate_is_closed(opt):
    ops, lib = _ops()
    grads, state = _grads()
    n = grads[0].numel()
    st = torch.tensor([R.INF, 0.5, 0.0, R.INF, 1.0, 0.0], device=DEV)
    init = (state['p'], state['m'], state['v'])
    bufs = [_Out((n,), t) for t in init]
    g = _in(grads[0])
    for triple in (0, 3):
        if opt == 'adam':
            lib.call('re2e_adam_step', bufs[0].ptr(), g.data_ptr(), bufs[1].ptr(), bufs[2].ptr(), n, 1e-3, 0.9, 0.999, 1e-8, 3, st.data_ptr() + 4 * triple)
        else:
            lib.call('re2e_adadelta_step', bufs[0].ptr(), g.data_ptr(), bufs[1].ptr(), bufs[2].ptr(), n, 0.95, 1e-8, 1.0, st.data_ptr() + 4 * triple)
        for b, t in zip(bufs, init):
            assert torch.equal(b.result(opt), t), 'stats[2] == 0: p and both state tensors stay bit-identical'


def test_zz_worst_distances_of_this_run():
    """One line per quantity: the worst HIP and fp32 CPU distance over whatever ran before in this process (the figures of the docstring)."""
    for q in sorted(WORST):
        print('WORST %-28s hip %.2e  fp32-cpu %.2e' % (q, WORST[q][0], WORST[q][1]))
