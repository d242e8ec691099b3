"""The attention steps dot, add, coverage (csrc/attstep.hip) and coverage_location (csrc/attloc.hip reading cov) under
ops.DecoderLoopFn against the float64 loops of tests/refs64_att.py: states, attention weights, d_enc, d_pre and every parameter
gradient the kind has, for every kind x shape of refs64_att.ATT_SHAPES x upstream gradient; the per-row forward step of the batched beam
search bit for bit against the per-utterance step; the shape limits' refusals.  The bars are the project's decoder-loop bars
(refs64.BAR_DEC_OUT / BAR_DEC_GRAD / ATOL_DEC_GRAD, gvec_b absolutely), each behind its ``margin_ok`` precondition."""
import ctypes
import functools

import pytest
import torch

import refs64 as R
import refs64_att as RA

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'


def _ops():
    from robust_e2e_gan_amd import ops, lib
    assert lib.query('re2e_device_ok') == 1, 'not a gfx950 device'
    return ops, lib


def _i32(v):
    return torch.as_tensor(v, dtype=torch.int32).to(DEV)


def _held(case, name, got, f64, f32, bar, atol=0.0):
    """Precondition (fp32 CPU within a quarter of the bar), then the HIP result within the bar of float64; prints both distances."""
    cpu = R.margin_ok(name, f32, f64, bar, atol)
    err = R.rel_err(got, f64)
    scale = f64.detach().double().abs().max().item()
    print('ERR %-46s %-16s hip %.2e  fp32-cpu %.2e  bar %.0e' % (case, name, err, cpu, bar))
    assert err * scale <= bar * scale + atol, '%s %s: HIP is %.3e of the max from float64 (bar %.1e, fp32 on the CPU: %.3e)' % (case, name, err, bar, cpu)


@functools.lru_cache(maxsize=None)
def _case(kind, shape):
    return RA.att_case(kind, shape)


@functools.lru_cache(maxsize=None)
def _refs(kind, shape, upstream):
    c = _case(kind, shape)
    return RA.att_ref_run(c, upstream=upstream), RA.att_ref_run(c, torch.float32, upstream)


def _sid(s):
    return 'x'.join(str(v) for v in s)


@pytest.mark.parametrize('upstream', R.DEC_UPSTREAM)
@pytest.mark.parametrize('shape', [s for s, _ in RA.ATT_SHAPES], ids=_sid)
@pytest.mark.parametrize('kind', RA.KINDS)
def test_decoder_loop_of_kind_against_float64(kind, shape, upstream):
    ops, lib = _ops()
    B, T, L1, E, A, D, C, Fh = shape
    c, (f64, f32) = _case(kind, shape), _refs(kind, shape, upstream)
    hm, pr = c['hmask'].to(DEV).requires_grad_(True), c['pre'].to(DEV).requires_grad_(True)
    Pm = {k: torch.nn.Parameter(v.to(DEV)) for k, v in c['Pm'].items()}
    if upstream == 'zs':
        zs, w = ops.DecoderLoopFn.apply(hm, pr, c['ids'].to(DEV), _i32(c['hlens']), L1, Pm, None, False, kind)
        assert not w.requires_grad
        up = (zs * c['gz'].to(DEV)).sum()
    else:
        zs, w = ops.DecoderLoopFn.apply(hm, pr, c['ids'].to(DEV), _i32(c['hlens']), L1, Pm, None, True, kind)
        up = (zs * c['gz'].to(DEV)).sum() + (w * c['gw'].to(DEV)).sum()
    assert zs.grad_fn.persist is False            # the persistent loop is location's alone
    up.backward()
    torch.cuda.synchronize()
    case = 'att-%s-%s-%s' % (kind, _sid(shape), upstream)
    _held(case, 'zs', zs, f64['zs'], f32['zs'], R.BAR_DEC_OUT)
    _held(case, 'w', w, f64['w'], f32['w'], R.BAR_DEC_OUT)
    if T == 1:
        assert torch.equal(w, torch.ones_like(w))
    got = dict(d_enc=hm.grad, d_pre=pr.grad, **{k: v.grad for k, v in Pm.items()})
    assert set(got) == {'d_enc', 'd_pre'} | set(RA.DEC_KEYS) | set(RA.ATT_KEYS[kind]) and all(v is not None for v in got.values())
    bad = []
    for k in sorted(got):
        if k == 'gvec_b':           # true gradient zero (a shift of the energies does not move a softmax): rounding noise of a sum over all frames
            err = got[k].abs().max().item()
            print('ERR %-46s %-16s hip %.2e (absolute; float64 %.1e)' % (case, k, err, f64[k].abs().max().item()))
            if not err <= 1e-5 * float(L1 * B):
                bad.append(k)
            continue
        try:
            _held(case, k, got[k], f64[k], f32[k], R.BAR_DEC_GRAD, R.ATOL_DEC_GRAD)
        except AssertionError as e:
            if 'input too hard' in str(e):
                raise
            bad.append(k)
    assert not bad, bad


def test_location_takes_the_kind_argument_and_launches_what_it_launched():
    """``kind='location'`` spelled out is the call without it: same outputs bit for bit, persistent form included."""
    ops, lib = _ops()
    shape = (2, 40, 3, 64, 64, 16, 12, 100)
    c = R.decoder_case(shape)
    outs = []
    for extra in ((), (None, False, 'location')):
        hm, pr = c['hmask'].to(DEV).requires_grad_(True), c['pre'].to(DEV).requires_grad_(True)
        Pm = {k: torch.nn.Parameter(v.to(DEV)) for k, v in c['Pm'].items()}
        zs, w = ops.DecoderLoopFn.apply(hm, pr, c['ids'].to(DEV), _i32(c['hlens']), c['L1'], Pm, *extra)
        (zs * c['gz'].to(DEV)).sum().backward()
        torch.cuda.synchronize()
        outs.append((zs.grad_fn.persist, zs.detach(), w.detach(), hm.grad, pr.grad, Pm['loc_conv'].grad, Pm['mlp_dec'].grad))
    assert outs[0][0] == outs[1][0] == ops.DECODER_PERSIST
    for a, b in zip(outs[0][1:], outs[1][1:]):
        assert torch.equal(a, b)


def _step_args(lib, kind, Pm, w_decT):
    opt = lambda k: Pm[k].data_ptr() if k in Pm else None
    return (opt('mlp_dec_b'), opt('wvec_w'), opt('wvec_b'), opt('gvec_w'), opt('gvec_b'))


@pytest.mark.parametrize('kind', RA.KINDS)
def test_rows_step_is_the_per_utterance_step_bit_for_bit(kind):
    """Seven rows over three utterances of 70 / 41 / 33 frames (pitch 70), rows sharing an utterance, each with its own decoder state and
    coverage row (a second step fed the first step's cov, and the first with cov_in = NULL): every row equals the per-utterance step
    called on that utterance alone with T = T_u; w and cov beyond T_u are written as 0."""
    ops, lib = _ops()
    from robust_e2e_gan_amd.lib import call, ATT_KINDS
    E, A, D, C, Fh = 68, 65, 20, 5, 8
    Ts, utt = [70, 41, 33], [0, 0, 1, 2, 2, 2, 1]
    U, nh, Tp = len(Ts), len(utt), max(Ts)
    c = RA.att_case(kind, (U, Tp, 1, E, A, D, C, Fh))
    Pm = {k: v.to(DEV).contiguous() for k, v in c['Pm'].items()}
    g = torch.Generator().manual_seed(3)
    enc, pre = torch.zeros(U, Tp, E), torch.zeros(U, Tp, A)
    for u, T in enumerate(Ts):
        enc[u, :T], pre[u, :T] = torch.randn(T, E, generator=g), torch.randn(T, A, generator=g)
    enc, pre = enc.to(DEV), pre.to(DEV)
    z = (torch.randn(nh, D, generator=g) * 0.5).to(DEV)
    w_decT = Pm['mlp_dec'].t().contiguous()
    covloc = kind == 'coverage_location'
    has_cov = kind.startswith('coverage')

    def step(pre_, enc_, z_, state, hl, n, T, utt_d=None):
        w, cx = torch.full((n, T), 7.0, device=DEV), torch.empty(n, E, device=DEV)
        dpj, e_scr, cov = torch.empty(n, A, device=DEV), torch.empty(n, T, device=DEV), torch.full((n, T), 7.0, device=DEV)
        st = state.data_ptr() if state is not None else None
        if covloc:
            conv = torch.empty(n, T, C, device=DEV)
            tail = (Pm['mlp_att'].data_ptr(), Pm['loc_conv'].data_ptr(), Pm['gvec_w'].data_ptr(), Pm['gvec_b'].data_ptr(), n, T, E, D, A, C, Fh,
                    w.data_ptr(), cx.data_ptr(), E, conv.data_ptr(), dpj.data_ptr(), e_scr.data_ptr())
            if utt_d is None:
                call('re2e_attloc_fwd', pre_.data_ptr(), enc_.data_ptr(), z_.data_ptr(), st, hl.data_ptr(), w_decT.data_ptr(), *tail)
            else:
                call('re2e_attloc_fwd_rows', pre_.data_ptr(), enc_.data_ptr(), U, hl.data_ptr(), utt_d.data_ptr(), z_.data_ptr(), st, w_decT.data_ptr(), *tail)
            call('re2e_attstep_cov_add', st, w.data_ptr(), hl.data_ptr(), utt_d.data_ptr() if utt_d is not None else None, U if utt_d is not None else n,
                 n, T, cov.data_ptr())
        else:
            tail = (*_step_args(lib, kind, Pm, w_decT), n, T, E, D, A, w.data_ptr(), cx.data_ptr(), E, cov.data_ptr() if has_cov else None, dpj.data_ptr(),
                    e_scr.data_ptr())
            if utt_d is None:
                call('re2e_attstep_fwd', ATT_KINDS[kind], pre_.data_ptr(), enc_.data_ptr(), z_.data_ptr(), st, hl.data_ptr(), w_decT.data_ptr(), *tail)
            else:
                call('re2e_attstep_fwd_rows', ATT_KINDS[kind], pre_.data_ptr(), enc_.data_ptr(), U, hl.data_ptr(), utt_d.data_ptr(), z_.data_ptr(), st,
                     w_decT.data_ptr(), *tail)
        torch.cuda.synchronize()
        return w, cx, (cov if has_cov else None)

    utt_d, tl = _i32(utt), _i32(Ts)
    w1, cx1, cov1 = step(pre, enc, z, None, tl, nh, Tp, utt_d)
    z2 = (torch.randn(nh, D, generator=g) * 0.5).to(DEV)
    w2, cx2, cov2 = step(pre, enc, z2, cov1, tl, nh, Tp, utt_d) if has_cov else (None, None, None)
    for r, u in enumerate(utt):
        T = Ts[u]
        pu, eu = pre[u:u + 1, :T].contiguous(), enc[u:u + 1, :T].contiguous()
        wa, ca, cva = step(pu, eu, z[r:r + 1].contiguous(), None, _i32([T]), 1, T)
        assert torch.equal(w1[r, :T], wa[0]) and torch.equal(cx1[r], ca[0]), (r, u)
        assert (w1[r, T:] == 0).all()
        if has_cov:
            assert torch.equal(cov1[r, :T], cva[0]) and (cov1[r, T:] == 0).all()
            wb, cb, cvb = step(pu, eu, z2[r:r + 1].contiguous(), cva, _i32([T]), 1, T)
            assert torch.equal(w2[r, :T], wb[0]) and torch.equal(cx2[r], cb[0]) and torch.equal(cov2[r, :T], cvb[0]), (r, u)
            assert (cov2[r, T:] == 0).all()
    # rows of one utterance with different decoder states differ (the map is not a broadcast)
    assert not torch.equal(w1[0], w1[1])


def _refused(lib, name, *args):
    fn = getattr(lib.load(), name)
    rc = fn(*args, None)
    return rc, lib.load().re2e_last_error().decode()


@pytest.mark.parametrize('what,B,T,E,D,A,kind,word', [
    ('adim', 1, 4, 8, 4, 321, 2, 'adim <= 320'),
    ('dunits', 1, 4, 8, 1025, 4, 2, 'dunits <= 1024'),
    ('eprojs', 1, 4, 6, 4, 4, 2, 'multiple of 4'),
    ('frames', 1, 40000, 4, 4, 4, 2, 'LDS'),
    ('location', 1, 4, 8, 4, 4, 0, 're2e_attloc'),
    ('coverage_location', 1, 4, 8, 4, 4, 4, 're2e_attloc'),
    ('unknown kind', 1, 4, 8, 4, 4, 9, 'unknown attention kind'),
])
def test_limits_refuse_with_a_message(what, B, T, E, D, A, kind, word):
    """Every limit of the header comment of csrc/attstep.hip: a refusal with a reason, before any launch."""
    ops, lib = _ops()
    f = lambda *s: torch.zeros(*s, device=DEV)
    pre, enc, z, w_decT = f(B, T, A), f(B, T, E), f(B, D), f(D, A)
    gv, gb, hl = f(A), f(1), _i32([T] * B)
    w, cx, dpj, e_scr = f(B, T), f(B, E), f(B, A), f(B, T)
    rc, msg = _refused(lib, 're2e_attstep_fwd', kind, pre.data_ptr(), enc.data_ptr(), z.data_ptr(), None, hl.data_ptr(), w_decT.data_ptr(), None, None, None,
                       gv.data_ptr(), gb.data_ptr(), B, T, E, D, A, w.data_ptr(), cx.data_ptr(), E, None, dpj.data_ptr(), e_scr.data_ptr())
    torch.cuda.synchronize()
    assert rc != 0 and word in msg, (rc, msg)
    if what in ('adim', 'eprojs', 'location', 'coverage_location', 'unknown kind'):
        ws = f(1 << 16)
        rc, msg = _refused(lib, 're2e_attstep_bwd', kind, pre.data_ptr(), enc.data_ptr(), None, w.data_ptr(), hl.data_ptr(), None, None, gv.data_ptr(),
                           dpj.data_ptr(), cx.data_ptr(), cx.data_ptr(), E, None, B, T, E, A, e_scr.data_ptr(), None, dpj.data_ptr(), ws.data_ptr(),
                           ctypes.c_size_t(ws.numel() * 4))
        assert rc != 0 and word in msg, (rc, msg)
    if what in ('adim', 'location', 'coverage_location', 'unknown kind'):
        rc, msg = _refused(lib, 're2e_attstep_dpre', kind, pre.data_ptr(), None, hl.data_ptr(), dpj.data_ptr(), e_scr.data_ptr(), None, None, gv.data_ptr(),
                           1, B, T, A, pre.data_ptr(), dpj.data_ptr(), ws.data_ptr(), ctypes.c_size_t(ws.numel() * 4))
        assert rc != 0 and word in msg, (rc, msg)


def test_missing_parameter_of_a_kind_is_refused():
    ops, lib = _ops()
    f = lambda *s: torch.zeros(*s, device=DEV)
    B, T, E, D, A = 1, 4, 8, 4, 4
    pre, enc, z, w_decT, hl = f(B, T, A), f(B, T, E), f(B, D), f(D, A), _i32([T])
    w, cx, dpj, e_scr, gv, gb = f(B, T), f(B, E), f(B, A), f(B, T), f(A), f(1)
    for kind, gvp in ((lib.ATT_DOT, gv.data_ptr()), (lib.ATT_ADD, None), (lib.ATT_COVERAGE, gv.data_ptr())):
        rc, msg = _refused(lib, 're2e_attstep_fwd', kind, pre.data_ptr(), enc.data_ptr(), z.data_ptr(), None, hl.data_ptr(), w_decT.data_ptr(), None, None, None,
                           gvp, gb.data_ptr(), B, T, E, D, A, w.data_ptr(), cx.data_ptr(), E, None, dpj.data_ptr(), e_scr.data_ptr())
        assert rc != 0 and ('null parameter' in msg or 'coverage needs' in msg), (kind, rc, msg)
