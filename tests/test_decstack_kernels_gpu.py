"""The upper layers of a multi-layer decoder (csrc/decstack.hip) under ops.DecoderUpperFn, and the full stacked loop through
ops.DecoderLoopFn + ops.DecoderUpperFn, against the float64 loops of tests/refs64_dlayers.py: top states, attention weights, d_enc, d_pre,
dZ0 and every parameter gradient of every layer, for every shape of refs64_dlayers.STACK_SHAPES x upstream gradient; the token step for n rows
bit for bit against the same rows launched singly; a single-layer loop called through the new optional argument bit for bit against the
call without it; the limits' refusals.  The bars are the project's decoder-loop bars (refs64.BAR_DEC_OUT / BAR_DEC_GRAD / ATOL_DEC_GRAD,
gvec_b absolutely), each behind its ``margin_ok`` precondition."""
import ctypes
import functools

import pytest
import torch

import refs64 as R
import refs64_dlayers as RD

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
SHAPES = [s for s, _ in RD.STACK_SHAPES]


def _ops():
    from robust_e2e_gan_amd import ops, lib
    assert lib.query('re2e_device_ok') == 1, 'not a gfx950 device'
    return ops, lib


def _i32(v):
    return torch.as_tensor(v, dtype=torch.int32).to(DEV)


def _sid(s):
    return 'x'.join(str(v) for v in s)


def _held(case, name, got, f64, f32, bar, atol=0.0):
    """Precondition (fp32 CPU within a quarter of the bar), then the HIP result within the bar of float64; prints both distances."""
    cpu = R.margin_ok(name, f32, f64, bar, atol)
    err = R.rel_err(got, f64)
    scale = f64.detach().double().abs().max().item()
    print('ERR %-34s %-12s hip %.2e  fp32-cpu %.2e  bar %.0e' % (case, name, err, cpu, bar))
    assert err * scale <= bar * scale + atol, '%s %s: HIP is %.3e of the max from float64 (bar %.1e, fp32 on the CPU: %.3e)' % (case, name, err, bar, cpu)


def _check(case, got, f64, f32, L1B):
    assert set(got) == set(f64) and all(v is not None for v in got.values()), set(got) ^ set(f64)
    bad = []
    for k in sorted(got):
        if k == 'gvec_b':           # true gradient zero: rounding noise of a sum over all frames (tests/test_attstep_kernels_gpu.py)
            if not got[k].abs().max().item() <= 1e-5 * float(L1B):
                bad.append(k)
            continue
        bar, atol = (R.BAR_DEC_OUT, 0.0) if k in ('z_top', 'w') else (R.BAR_DEC_GRAD, R.ATOL_DEC_GRAD)
        try:
            _held(case, k, got[k], f64[k], f32[k], bar, atol)
        except AssertionError as e:
            if 'input too hard' in str(e):
                raise
            bad.append(k)
    assert not bad, bad


def _layers_dev(layers):
    return [{k: torch.nn.Parameter(v.to(DEV).contiguous()) for k, v in lay.items()} for lay in layers]


def _layer_grads(lays):
    return {'l%d.%s' % (l + 1, k): lay[k].grad for l, lay in enumerate(lays) for k in RD.UPPER_KEYS}


@functools.lru_cache(maxsize=None)
def _stack_refs(shape):
    c = RD.stack_case(shape)
    return c, RD.stack_ref_run(c), RD.stack_ref_run(c, torch.float32)


@functools.lru_cache(maxsize=None)
def _loop_refs(shape, upstream):
    c = RD.loop_case(shape)
    return c, RD.loop_ref_run(c, upstream=upstream), RD.loop_ref_run(c, torch.float32, upstream)


@pytest.mark.parametrize('shape', SHAPES, ids=_sid)
def test_upper_layers_against_float64(shape):
    ops, lib = _ops()
    B, L1, D, nl = shape
    c, f64, f32 = _stack_refs(shape)
    z0 = c['z0'].to(DEV).requires_grad_(True)
    lays = _layers_dev(c['layers'])
    top = ops.DecoderUpperFn.apply(z0, lays)
    assert tuple(top.shape) == (L1, B, D)
    (top * c['gz'].to(DEV)).sum().backward()
    torch.cuda.synchronize()
    _check('stack-' + _sid(shape), dict(z_top=top, dZ0=z0.grad, **_layer_grads(lays)), f64, f32, L1 * B)


@pytest.mark.parametrize('upstream', R.DEC_UPSTREAM)
@pytest.mark.parametrize('shape', SHAPES, ids=_sid)
def test_stacked_loop_against_float64(shape, upstream):
    """DecoderLoopFn (layer 0, unchanged) then DecoderUpperFn, as the teacher-forced model path composes them."""
    ops, lib = _ops()
    B, L1, D, nl = shape
    c, f64, f32 = _loop_refs(shape, upstream)
    hm, pr = c['hmask'].to(DEV).requires_grad_(True), c['pre'].to(DEV).requires_grad_(True)
    Pm = {k: torch.nn.Parameter(v.to(DEV)) for k, v in c['Pm'].items()}
    lays = _layers_dev(c['layers'])
    z0, w = ops.DecoderLoopFn.apply(hm, pr, c['ids'].to(DEV), _i32(c['hlens']), L1, Pm, None, upstream == 'zs+w')
    top = ops.DecoderUpperFn.apply(z0, lays)
    up = (top * c['gz'].to(DEV)).sum()
    if upstream == 'zs+w':
        up = up + (w * c['gw'].to(DEV)).sum()
    up.backward()
    torch.cuda.synchronize()
    got = dict(z_top=top, w=w, d_enc=hm.grad, d_pre=pr.grad, **{k: v.grad for k, v in Pm.items()}, **_layer_grads(lays))
    _check('loop-%s-%s' % (_sid(shape), upstream), got, f64, f32, L1 * B)


@pytest.mark.parametrize('shape', [(5, 6, 12, 3), (2, 3, 300, 2)], ids=_sid)
def test_loop_with_upper_argument_is_the_composition(shape):
    """DecoderLoopFn given ``upper`` (no sampled steps) returns the top layer's states and runs the two-phase backward itself: bit for bit
    what DecoderLoopFn followed by DecoderUpperFn gives, the persistent layer-0 loop included."""
    ops, lib = _ops()
    B, L1, D, nl = shape
    c = RD.loop_case(shape)
    outs = []
    for fused in (False, True):
        hm, pr = c['hmask'].to(DEV).requires_grad_(True), c['pre'].to(DEV).requires_grad_(True)
        Pm = {k: torch.nn.Parameter(v.to(DEV)) for k, v in c['Pm'].items()}
        lays = _layers_dev(c['layers'])
        if fused:
            top, w = ops.DecoderLoopFn.apply(hm, pr, c['ids'].to(DEV), _i32(c['hlens']), L1, Pm, None, False, 'location', lays)
            persist = top.grad_fn.persist
        else:
            z0, w = ops.DecoderLoopFn.apply(hm, pr, c['ids'].to(DEV), _i32(c['hlens']), L1, Pm)
            persist = z0.grad_fn.persist
            top = ops.DecoderUpperFn.apply(z0, lays)
        (top * c['gz'].to(DEV)).sum().backward()
        torch.cuda.synchronize()
        outs.append((persist, top.detach(), w.detach(), hm.grad, pr.grad, Pm['w_hh'].grad, Pm['loc_conv'].grad, *_layer_grads(lays).values()))
    assert outs[0][0] == outs[1][0] == ops.DECODER_PERSIST
    for a, b in zip(outs[0][1:], outs[1][1:]):
        assert torch.equal(a, b)


@pytest.mark.parametrize('n', [1, 12, 64, 193])
@pytest.mark.parametrize('D', [300, 20])
def test_token_step_rows_are_independent_bit_for_bit(n, D):
    """re2e_dec_upper_step for n rows against the same rows launched one at a time: z, c and the activated gates, every bit; and against
    float64 within the decoder-state bar."""
    ops, lib = _ops()
    g = torch.Generator().manual_seed(100 * n + D)
    r = lambda *s, scale=1.0: torch.randn(*s, generator=g) * scale
    lay = dict(w_ih=r(4 * D, D, scale=0.08), w_hh=r(4 * D, D, scale=0.08), b_ih=r(4 * D, scale=0.1), b_hh=r(4 * D, scale=0.1))
    x, zp, cp = torch.tanh(r(n, D)), torch.tanh(r(n, D)) * 0.8, r(n, D)
    d = {k: v.to(DEV) for k, v in lay.items()}
    xd, zd, cd = x.to(DEV), zp.to(DEV), cp.to(DEV)

    def step(rows):
        m = rows.stop - rows.start
        gates, z, c = (torch.full((m, 4 * D), 7.0, device=DEV), torch.full((m, D), 7.0, device=DEV), torch.full((m, D), 7.0, device=DEV))
        lib.call('re2e_dec_upper_step', xd[rows].data_ptr(), d['w_ih'].data_ptr(), d['w_hh'].data_ptr(), d['b_ih'].data_ptr(), d['b_hh'].data_ptr(),
                 zd[rows].data_ptr(), cd[rows].data_ptr(), gates.data_ptr(), z.data_ptr(), c.data_ptr(), m, D)
        return gates, z, c

    ga, za, ca = step(slice(0, n))
    singles = [step(slice(i, i + 1)) for i in range(0, n, max(1, n // 24))] + [step(slice(n - 1, n))]
    rows = list(range(0, n, max(1, n // 24))) + [n - 1]
    torch.cuda.synchronize()
    for i, (g1, z1, c1) in zip(rows, singles):
        assert torch.equal(ga[i], g1[0]) and torch.equal(za[i], z1[0]) and torch.equal(ca[i], c1[0]), i
    # no output without the gates: the search's call
    z2, c2 = torch.empty(n, D, device=DEV), torch.empty(n, D, device=DEV)
    lib.call('re2e_dec_upper_step', xd.data_ptr(), d['w_ih'].data_ptr(), d['w_hh'].data_ptr(), d['b_ih'].data_ptr(), d['b_hh'].data_ptr(), zd.data_ptr(),
             cd.data_ptr(), None, z2.data_ptr(), c2.data_ptr(), n, D)
    torch.cuda.synchronize()
    assert torch.equal(z2, za) and torch.equal(c2, ca)

    def ref(dt):
        gi, gf, gg, go = (x.to(dt) @ lay['w_ih'].to(dt).t() + zp.to(dt) @ lay['w_hh'].to(dt).t() + lay['b_ih'].to(dt) + lay['b_hh'].to(dt)).chunk(4, 1)
        c = torch.sigmoid(gf) * cp.to(dt) + torch.sigmoid(gi) * torch.tanh(gg)
        return torch.sigmoid(go) * torch.tanh(c), c
    (z64, c64), (z32, c32) = ref(torch.float64), ref(torch.float32)
    _held('step-n%d-D%d' % (n, D), 'z', za, z64, z32, R.BAR_DEC_OUT)
    _held('step-n%d-D%d' % (n, D), 'c', ca, c64, c32, R.BAR_DEC_OUT)


def test_one_layer_through_the_new_argument_launches_what_it_launched():
    """``upper`` given as None or as an empty list is the call without it: same outputs bit for bit, persistent form included; also with
    sampled steps (the launch-per-step loop)."""
    ops, lib = _ops()
    shape = (2, 40, 3, 64, 64, 16, 12, 100)
    c = R.decoder_case(shape)
    g = torch.Generator().manual_seed(4)
    out_w, out_b = (torch.randn(50, 16, generator=g) * 0.5).to(DEV), (torch.randn(50, generator=g) * 0.1).to(DEV)
    for steps in (None, (False, True, True)):
        outs = []
        for extra in ((), (False, 'location', None), (False, 'location', [])):
            hm, pr = c['hmask'].to(DEV).requires_grad_(True), c['pre'].to(DEV).requires_grad_(True)
            Pm = {k: torch.nn.Parameter(v.to(DEV)) for k, v in c['Pm'].items()}
            Pm.update(out_w=out_w, out_b=out_b)
            zs, w = ops.DecoderLoopFn.apply(hm, pr, c['ids'].to(DEV), _i32(c['hlens']), c['L1'], Pm, steps, *extra)
            (zs * c['gz'].to(DEV)).sum().backward()
            torch.cuda.synchronize()
            outs.append((zs.grad_fn.persist, zs.grad_fn.ids.clone(), zs.detach(), w.detach(), hm.grad, pr.grad, Pm['loc_conv'].grad, Pm['mlp_dec'].grad,
                         Pm['w_ih'].grad))
        assert outs[0][0] == outs[1][0] == outs[2][0] == (ops.DECODER_PERSIST and steps is None)
        for other in outs[1:]:
            for a, b in zip(outs[0][1:], other[1:]):
                assert torch.equal(a, b)


def test_sampled_loop_runs_the_token_step_inside_the_loop():
    """Sampled steps with two upper layers: the tokens fed are the arg-max of the output layer on the TOP layer's previous state (replayed in
    float64 from the device's states, with a margin that rules a rounding tie out), and states, weights and all gradients are those of the
    float64 loop teacher-forced on these tokens."""
    ops, lib = _ops()
    shape = (5, 6, 12, 3)
    B, L1, D, nl = shape
    c = RD.loop_case(shape)
    g = torch.Generator().manual_seed(12)          # (the two best logits of every sampled step are 5e-2 apart in float64)
    out_w, out_b = torch.randn(50, D, generator=g) * 2.0, torch.randn(50, generator=g) * 0.1
    steps = (False, True, False, True, True, True)
    hm, pr = c['hmask'].to(DEV).requires_grad_(True), c['pre'].to(DEV).requires_grad_(True)
    Pm = {k: torch.nn.Parameter(v.to(DEV)) for k, v in c['Pm'].items()}
    Pm.update(out_w=out_w.to(DEV), out_b=out_b.to(DEV))
    lays = _layers_dev(c['layers'])
    top, w = ops.DecoderLoopFn.apply(hm, pr, c['ids'].to(DEV), _i32(c['hlens']), L1, Pm, steps, False, 'location', lays)
    assert top.grad_fn.persist is False
    fed = top.grad_fn.ids.view(L1, B).cpu()
    (top * c['gz'].to(DEV)).sum().backward()
    torch.cuda.synchronize()
    own, margin = RD.sampled_tokens(top.detach().cpu().double(), c['ids'], out_w.double(), out_b.double(), steps)
    assert margin > 1e-2, margin
    assert torch.equal(own, fed) and not torch.equal(fed, c['ids']) and torch.equal(fed[2], c['ids'][2])
    case = dict(c, ids=fed)
    f64, f32 = RD.loop_ref_run(case), RD.loop_ref_run(case, torch.float32)
    # the float64 loop's own states choose the same tokens: the comparison is not one of two label sequences
    own64, _ = RD.sampled_tokens(f64['z_top'], c['ids'], out_w.double(), out_b.double(), steps)
    assert torch.equal(own64, fed)
    got = dict(z_top=top, w=w, d_enc=hm.grad, d_pre=pr.grad, **{k: Pm[k].grad for k in c['Pm']}, **_layer_grads(lays))
    _check('sampled-' + _sid(shape), got, f64, f32, L1 * B)


def _raw(lib, name, *args):
    rc = getattr(lib.load(), name)(*args, None)
    return rc, lib.load().re2e_last_error().decode()


@pytest.mark.parametrize('D,word', [(6, 'multiple of 4'), (1028, 'at most 1024')])
def test_limits_refuse_with_a_message(D, word):
    """D % 4 != 0 and D > 1024: RE2E_EUNSUPPORTED with a reason from all three entry points, nothing launched."""
    ops, lib = _ops()
    f = lambda *s: torch.zeros(*s, device=DEV)
    B, L1 = 2, 2
    w, b, x, g, z = f(4 * D, D), f(4 * D), f(B, D), f(L1, B, 4 * D), f(L1 + 1, B, D)
    rc, msg = _raw(lib, 're2e_dec_upper_step', x.data_ptr(), w.data_ptr(), w.data_ptr(), b.data_ptr(), b.data_ptr(), x.data_ptr(), x.data_ptr(), None,
                   z[0].data_ptr(), z[1].data_ptr(), B, D)
    assert rc == lib.EUNSUPPORTED and word in msg, (rc, msg)
    rc, msg = _raw(lib, 're2e_dec_upper_seq_fwd', g.data_ptr(), w.data_ptr(), z.data_ptr(), z.data_ptr(), L1, B, D)
    assert rc == lib.EUNSUPPORTED and word in msg, (rc, msg)
    ws = f(4 * B * D)
    rc, msg = _raw(lib, 're2e_dec_upper_seq_bwd', g.data_ptr(), z.data_ptr(), z.data_ptr(), w.data_ptr(), g.data_ptr(), L1, B, D, ws.data_ptr(),
                   ctypes.c_size_t(ws.numel() * 4))
    assert rc == lib.EUNSUPPORTED and word in msg, (rc, msg)
    torch.cuda.synchronize()


@pytest.mark.parametrize('shape', [(3, 4, 14, 3), (2, 2, 1028, 2)], ids=_sid)
def test_widths_outside_the_kernels_run_over_the_general_entry_points(shape):
    """D % 4 != 0 (the tiny fixtures' dunits = 14) and D > 1024: ops runs the same steps over re2e_gemm + re2e_lstm_cell_fwd / _bwd, held to
    the same bars."""
    ops, lib = _ops()
    B, L1, D, nl = shape
    assert not ops._upper_fused(D)
    c, f64, f32 = _stack_refs(shape)
    z0 = c['z0'].to(DEV).requires_grad_(True)
    lays = _layers_dev(c['layers'])
    top = ops.DecoderUpperFn.apply(z0, lays)
    (top * c['gz'].to(DEV)).sum().backward()
    torch.cuda.synchronize()
    _check('stack-' + _sid(shape), dict(z_top=top, dZ0=z0.grad, **_layer_grads(lays)), f64, f32, L1 * B)


def test_widest_layer_runs():
    """D = 1024, the limit: the backward's row tile of d(gates) is 128 KiB of LDS.  One layer, three rows, two tokens against float64."""
    ops, lib = _ops()
    c = RD.stack_case((3, 2, 1024, 2))
    f64, f32 = RD.stack_ref_run(c), RD.stack_ref_run(c, torch.float32)
    z0 = c['z0'].to(DEV).requires_grad_(True)
    lays = _layers_dev(c['layers'])
    top = ops.DecoderUpperFn.apply(z0, lays)
    (top * c['gz'].to(DEV)).sum().backward()
    torch.cuda.synchronize()
    _check('stack-3x2x1024x2', dict(z_top=top, dZ0=z0.grad, **_layer_grads(lays)), f64, f32, 6)
