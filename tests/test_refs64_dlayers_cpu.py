"""Pins tests/refs64_dlayers.py (CPU only) and the host side of the multi-layer decoder (dlayers > 1):

- the written-out float64 stacked loop against the golden vectors the reference's own E2E produced with dlayers 2 and 3
  (tests/golden/dlayers_tiny.npz): the teacher-forced ``loss_att`` and the greedy attention dump;
- against a second derivation through torch.nn.LSTMCell, values and every gradient;
- for every input of tests/test_decstack_kernels_gpu.py, that torch's own fp32 run of the reference stays within a quarter of the bar the
  HIP kernels are held to there;
- what E2E builds for dlayers 1, 2, 3, its state_dict names and shapes against the fixture's, load_state_dict round trips, and the refusals."""
import argparse
import functools
import os

import numpy as np
import pytest
import torch

import refs64 as R
import refs64_att as RA
import refs64_dlayers as RD
from test_refs64_att_cpu import loop_inputs, split_targets

MODELS = (('loc2', 'location', 2), ('loc3', 'location', 3), ('cov2', 'coverage', 2))
LOC_KEYS = dict(mlp_dec='att.mlp_dec.weight', mlp_att='att.mlp_att.weight', loc_conv='att.loc_conv.weight', gvec_w='att.gvec.weight', gvec_b='att.gvec.bias')


def _fx(golden_dir, name):
    return dict(np.load(os.path.join(golden_dir, name), allow_pickle=False))


def fixture_model(golden_dir, tag):
    """Reference-named parameters of the fixture's model ``tag``: e2e_tiny.npz's (coverage: with att_types_tiny.npz's attention), the
    fixture's own ``dec.decoder.{1,2}.*`` -> (parameters, the state_dict a model loads, dlayers_tiny.npz, att_types_tiny.npz)."""
    kind, nl = {t: (k, n) for t, k, n in MODELS}[tag]
    base, att, fx = _fx(golden_dir, 'e2e_tiny.npz'), _fx(golden_dir, 'att_types_tiny.npz'), _fx(golden_dir, 'dlayers_tiny.npz')
    p = {k[2:]: torch.from_numpy(v) for k, v in base.items() if k.startswith('p.') and not k.startswith('p.dec.att.')}
    if kind != 'location':
        p = {k: v for k, v in p.items() if not k.startswith('att.')}
        p.update({k[len(kind) + 3:]: torch.from_numpy(v) for k, v in att.items() if k.startswith(kind + '.p.att.')})
    p.update({k[len(tag) + 3:]: torch.from_numpy(v) for k, v in fx.items() if k.startswith(tag + '.p.')})
    sd = dict(p)
    sd.update({'dec.' + k: v for k, v in p.items() if k.startswith('att.')})
    return p, sd, fx, att


def stacked_inputs(kind, p, hpad, hlens, ys, eos, dtype):
    """loop_inputs of layer 0 (``location``: with AttLoc's parameters) plus the upper layers of ``p``."""
    if kind == 'location':
        hmask, pre, ids, tgt, L1, Pm = loop_inputs('add', p, hpad, hlens, ys, eos, dtype)
        Pm = {k: v for k, v in Pm.items() if k in RA.DEC_KEYS}
        Pm.update({k: p[n].detach().to(dtype) for k, n in LOC_KEYS.items()})
    else:
        hmask, pre, ids, tgt, L1, Pm = loop_inputs(kind, p, hpad, hlens, ys, eos, dtype)
    layers, l = [], 1
    while 'dec.decoder.%d.weight_ih' % l in p:
        q = 'dec.decoder.%d.' % l
        layers.append({k: p[q + n].detach().to(dtype) for k, n in (('w_ih', 'weight_ih'), ('w_hh', 'weight_hh'), ('b_ih', 'bias_ih'), ('b_hh', 'bias_hh'))})
        l += 1
    return hmask, pre, ids, tgt, L1, Pm, layers


def _close(name, got, ref, tol):
    err = (got.double() - ref.double()).abs().max().item()
    scale = ref.double().abs().max().item()
    assert err <= tol * scale + 1e-6, '%s: max err %.3e vs scale %.3e' % (name, err, scale)


@pytest.mark.parametrize('tag', [t for t, _, _ in MODELS])
def test_stacked_loop_reproduces_the_reference(golden_dir, tag):
    kind, nl = {t: (k, n) for t, k, n in MODELS}[tag]
    p, _, fx, att = fixture_model(golden_dir, tag)
    hlens, tl, ys = att['add.hlens'].tolist(), att['tlens'].tolist(), split_targets(att)
    hmask, pre, ids, tgt, L1, Pm, layers = stacked_inputs(kind, p, torch.from_numpy(att['add.hpad']), hlens, ys, 11, torch.float64)
    assert len(layers) == nl - 1
    out_w, out_b = p['dec.output.weight'].double(), p['dec.output.bias'].double()
    # teacher forced: the loss the reference recorded, through the cross-entropy reference on the TOP layer's states
    z0, _ = RD.layer0_ref(kind, hmask, pre, ids, hlens, L1, Pm)
    top = RD.upper_ref(z0, layers)[-1]
    loss, _, _, _ = R.ce_ref(top.reshape(L1 * len(hlens), -1) @ out_w.t() + out_b, tgt.reshape(-1), float(np.mean([n + 1 for n in tl])) - 1.0)
    _close('loss_att', loss.view(1), torch.from_numpy(fx[tag + '.loss_att']).view(1), 1e-4)
    lone, _, _, _ = R.ce_ref(z0.reshape(L1 * len(hlens), -1) @ out_w.t() + out_b, tgt.reshape(-1), float(np.mean([n + 1 for n in tl])) - 1.0)
    assert abs(float(lone) - float(fx[tag + '.loss_att'])) > 1e-3          # the upper layers matter
    # greedy (calculate_all_attentions): iterate the fed tokens to their fixed point (token i depends on tokens < i only), then the dump
    steps = tuple(i > 0 for i in range(L1))
    fed = ids.clone()
    for _ in range(L1):
        z0, w = RD.layer0_ref(kind, hmask, pre, fed, hlens, L1, Pm)
        new, _ = RD.sampled_tokens(RD.upper_ref(z0, layers)[-1], ids, out_w, out_b, steps)
        if torch.equal(new, fed):
            break
        fed = new
    else:
        raise AssertionError('greedy tokens did not settle')
    _close('att', w.transpose(0, 1), torch.from_numpy(fx[tag + '.att']), 1e-4)


SMALL = [s for s, _ in RD.STACK_SHAPES if s[0] * s[2] <= 33 * 68]


@pytest.mark.parametrize('shape', SMALL, ids=lambda s: 'x'.join(str(v) for v in s))
def test_stack_ref_against_torch_lstmcell(shape):
    c = RD.stack_case(shape)
    a, b = RD.stack_ref_run(c), RD.stack_ref_run(c, stack=RD.upper_modules)
    assert set(a) == set(b) == {'z_top', 'dZ0'} | {'l%d.%s' % (l, k) for l in range(1, shape[3]) for k in RD.UPPER_KEYS}
    for k in sorted(a):
        assert a[k].shape == b[k].shape, k
        scale = max(a[k].abs().max().item(), 1e-30)
        assert (a[k] - b[k]).abs().max().item() <= 1e-10 * scale + 1e-13, (k, (a[k] - b[k]).abs().max().item(), scale)


@functools.lru_cache(maxsize=None)
def stack_refs(shape):
    c = RD.stack_case(shape)
    return RD.stack_ref_run(c), RD.stack_ref_run(c, torch.float32)


@functools.lru_cache(maxsize=None)
def loop_refs(shape, upstream):
    c = RD.loop_case(shape)
    return RD.loop_ref_run(c, upstream=upstream), RD.loop_ref_run(c, torch.float32, upstream)


def check_margins(f64, f32):
    for k in sorted(f64):
        if k == 'gvec_b':
            assert f64[k].abs().max().item() < 1e-12           # analytically zero
        elif k in ('z_top', 'w'):
            R.margin_ok(k, f32[k], f64[k], R.BAR_DEC_OUT)
        else:
            R.margin_ok(k, f32[k], f64[k], R.BAR_DEC_GRAD, R.ATOL_DEC_GRAD)


@pytest.mark.parametrize('shape', [s for s, _ in RD.STACK_SHAPES], ids=lambda s: 'x'.join(str(v) for v in s))
def test_bars_are_meaningful_on_the_stack_inputs(shape):
    check_margins(*stack_refs(shape))


@pytest.mark.parametrize('upstream', R.DEC_UPSTREAM)
@pytest.mark.parametrize('shape', [s for s, _ in RD.STACK_SHAPES], ids=lambda s: 'x'.join(str(v) for v in s))
def test_bars_are_meaningful_on_the_loop_inputs(shape, upstream):
    check_margins(*loop_refs(shape, upstream))


# ---------------------------------------------------------------------------------------------
# host side
# ---------------------------------------------------------------------------------------------
def _opt(atype='location', **kw):
    import __graft_entry__ as g
    return argparse.Namespace(**{**vars(g._tiny_opt()), 'atype': atype, **kw})


@pytest.mark.parametrize('tag', [t for t, _, _ in MODELS])
def test_e2e_builds_the_layers_with_the_reference_names(golden_dir, tag):
    from robust_e2e_gan_amd.model.e2e_model import E2E, ShareE2E
    kind, nl = {t: (k, n) for t, k, n in MODELS}[tag]
    _, sd, _, _ = fixture_model(golden_dir, tag)
    want = {k: tuple(v.shape) for k, v in sd.items()}
    for l in range(1, nl):
        assert want['dec.decoder.%d.weight_ih' % l] == (56, 14) and want['dec.decoder.%d.weight_hh' % l] == (56, 14)
        assert want['dec.decoder.%d.bias_ih' % l] == (56,) and want['dec.decoder.%d.bias_hh' % l] == (56,)
    assert 'dec.decoder.%d.weight_ih' % nl not in want
    for model in (E2E, ShareE2E):
        m = model(_opt(kind, dlayers=nl))
        have = {k: tuple(v.shape) for k, v in m.state_dict().items()}
        assert have == want, set(have) ^ set(want)
        assert m.dec.dlayers == nl and len(m.dec.decoder) == nl


@pytest.mark.parametrize('tag', [t for t, _, _ in MODELS])
def test_state_dict_round_trip(golden_dir, tag):
    from robust_e2e_gan_amd.model.e2e_model import E2E
    kind, nl = {t: (k, n) for t, k, n in MODELS}[tag]
    _, sd, _, _ = fixture_model(golden_dir, tag)
    m = E2E(_opt(kind, dlayers=nl))
    m.load_state_dict(sd, strict=True)
    back = m.state_dict()
    assert set(back) == set(sd) and all(torch.equal(back[k], sd[k]) for k in sd)
    m2 = E2E(_opt(kind, dlayers=nl))
    m2.load_state_dict(back, strict=True)
    assert all(torch.equal(a, b) for a, b in zip(m.parameters(), m2.parameters()))
    # a deeper checkpoint does not load into a shallower model, nor the other way round
    with pytest.raises(RuntimeError):
        E2E(_opt(kind, dlayers=nl - 1)).load_state_dict(sd, strict=True)
    with pytest.raises(RuntimeError):
        E2E(_opt(kind, dlayers=nl + 1)).load_state_dict(sd, strict=True)


def test_one_layer_has_exactly_the_keys_it_had(golden_dir):
    from robust_e2e_gan_amd.model.e2e_model import E2E
    base = _fx(golden_dir, 'e2e_tiny.npz')
    want = {k[2:]: tuple(v.shape) for k, v in base.items() if k.startswith('p.')}
    m = E2E(_opt())
    assert m.dec.dlayers == 1
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == want
    assert [k for k in want if k.startswith('dec.decoder.')] == ['dec.decoder.0.weight_ih', 'dec.decoder.0.weight_hh', 'dec.decoder.0.bias_ih',
                                                                 'dec.decoder.0.bias_hh']


@pytest.mark.parametrize('dlayers', [0, -1])
def test_no_layers_is_refused(dlayers):
    from robust_e2e_gan_amd.lib import Re2eError
    from robust_e2e_gan_amd.model.e2e_model import E2E
    with pytest.raises(Re2eError, match='at least one layer'):
        E2E(_opt(dlayers=dlayers))


def test_decoder_collects_the_layers_from_a_parameter_dict(golden_dir):
    from robust_e2e_gan_amd.model import e2e_decoder as D
    for tag, kind, nl in MODELS:
        p, _, _, _ = fixture_model(golden_dir, tag)
        lays = D.upper_layers(p)
        assert len(lays) == nl - 1 and all(set(lay) == set(RD.UPPER_KEYS) for lay in lays)
        assert lays[0]['w_ih'] is p['dec.decoder.1.weight_ih'] and lays[-1]['b_hh'] is p['dec.decoder.%d.bias_hh' % (nl - 1)]
        assert len(D.upper_layers({'x.' + k: v for k, v in p.items()}, 'x.')) == nl - 1
    assert D.upper_layers({'dec.decoder.0.weight_ih': None}) == []

