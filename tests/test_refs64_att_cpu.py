"""Pins tests/refs64_att.py (CPU only) and the host side of the attention types dot, add, coverage and coverage_location:

- the written-out float64 loops against the golden vectors the reference's own AttDot / AttAdd / AttCov / AttCovLoc produced
  (tests/golden/att_types_tiny.npz): the greedy attention dump and the teacher-forced ``loss_att``;
- against a second derivation through torch.nn modules, values and every gradient;
- for every input of tests/test_attstep_kernels_gpu.py, that torch's own fp32 run of the reference stays within a quarter of the bar
  the HIP kernels are held to there;
- what E2E builds and still refuses, its state_dict names and shapes against the fixture's, and load_state_dict round trips."""
import argparse
import functools
import os

import numpy as np
import pytest
import torch

import refs64 as R
import refs64_att as RA


def _fx(golden_dir, name):
    return dict(np.load(os.path.join(golden_dir, name), allow_pickle=False))


def fixture_params(golden_dir, kind):
    """Reference-named parameters of the fixture's model of ``kind``: e2e_tiny.npz's encoder / CTC / decoder, the fixture's own ``att.*``."""
    base, fx = _fx(golden_dir, 'e2e_tiny.npz'), _fx(golden_dir, 'att_types_tiny.npz')
    p = {k[2:]: torch.from_numpy(v) for k, v in base.items() if k.startswith('p.') and not k.startswith(('p.att.', 'p.dec.att.'))}
    p.update({k[len(kind) + 3:]: torch.from_numpy(v) for k, v in fx.items() if k.startswith(kind + '.p.att.')})
    return p, fx


def loop_inputs(kind, p, hpad, hlens, ys, eos, dtype):
    """What model/e2e_decoder.py hands to the loop of ``kind``."""
    B, T, _ = hpad.shape
    L1 = max(len(y) for y in ys) + 1
    ids_in = torch.full((B, L1), eos, dtype=torch.long)
    ids_out = torch.full((B, L1), -1, dtype=torch.long)
    for b, y in enumerate(ys):
        ids_in[b, 1:len(y) + 1] = y
        ids_out[b, :len(y)] = y
        ids_out[b, len(y)] = eos
    d = lambda k: p[k].detach().to(dtype)
    hmask = hpad.detach().to(dtype) * (torch.arange(T).unsqueeze(0) < torch.tensor(hlens).unsqueeze(1)).unsqueeze(2).to(dtype)
    pre = hmask @ d('att.mlp_enc.weight').t() + d('att.mlp_enc.bias')
    if kind == 'dot':
        pre = torch.tanh(pre)
    names = dict(mlp_dec='att.mlp_dec.weight', mlp_dec_b='att.mlp_dec.bias', wvec_w='att.wvec.weight', wvec_b='att.wvec.bias',
                 mlp_att='att.mlp_att.weight', loc_conv='att.loc_conv.weight', gvec_w='att.gvec.weight', gvec_b='att.gvec.bias')
    Pm = dict(embed=d('dec.embed.weight'), w_ih=d('dec.decoder.0.weight_ih'), w_hh=d('dec.decoder.0.weight_hh'), b_ih=d('dec.decoder.0.bias_ih'),
              b_hh=d('dec.decoder.0.bias_hh'))
    Pm.update({k: d(names[k]) for k in RA.ATT_KEYS[kind]})
    return hmask, pre, ids_in.t().contiguous(), ids_out.t().contiguous(), L1, Pm


def dump_key(kind):
    """The fixture's attention weights of every step: upstream's dump, but for the coverage types, whose dump repeats the last step (the
    attention returns ONE list that it grows in place), the rows of that list."""
    return kind + ('.att_steps' if kind.startswith('coverage') else '.att')


def split_targets(fx):
    ys, o = [], 0
    for n in fx['tlens'].tolist():
        ys.append(torch.from_numpy(fx['targets'][o:o + n]))
        o += n
    return ys


def _close(name, got, ref, tol):
    err = (got.double() - ref.double()).abs().max().item()
    scale = ref.double().abs().max().item()
    assert err <= tol * scale + 1e-6, '%s: max err %.3e vs scale %.3e' % (name, err, scale)


@pytest.mark.parametrize('kind', RA.KINDS)
def test_loop_ref_reproduces_the_reference(golden_dir, kind):
    p, fx = fixture_params(golden_dir, kind)
    hlens, tl, ys = fx[kind + '.hlens'].tolist(), fx['tlens'].tolist(), split_targets(fx)
    hmask, pre, ids, tgt, L1, Pm = loop_inputs(kind, p, torch.from_numpy(fx[kind + '.hpad']), hlens, ys, 11, torch.float64)
    # teacher forced: the loss the reference recorded, through the cross-entropy reference
    zs, w, fed = RA.att_loop_ref(kind, hmask, pre, ids, hlens, L1, Pm)
    assert torch.equal(fed, ids)
    out_w, out_b = p['dec.output.weight'].double(), p['dec.output.bias'].double()
    loss, _, _, _ = R.ce_ref(zs.reshape(L1 * len(hlens), -1) @ out_w.t() + out_b, tgt.reshape(-1), float(np.mean([n + 1 for n in tl])) - 1.0)
    _close('loss_att', loss.view(1), torch.from_numpy(fx[kind + '.loss_att']).view(1), 1e-4)
    # greedy (calculate_all_attentions): the dump
    _, wg, _ = RA.att_loop_ref(kind, hmask, pre, ids, hlens, L1, Pm, out_w, out_b, tuple(i > 0 for i in range(L1)))
    _close('att', wg.transpose(0, 1), torch.from_numpy(fx[dump_key(kind)]), 1e-4)
    if kind.startswith('coverage'):
        # what upstream's own dump holds for these two types: the last step's row, L1 times (make_fixtures_att.py run_type)
        assert np.array_equal(fx[kind + '.att'], np.repeat(fx[kind + '.att_steps'][:, -1:], L1, 1))


SMALL = [s for s, _ in RA.ATT_SHAPES if s[1] * s[3] * s[4] <= 33 * 68 * 65]


@pytest.mark.parametrize('upstream', R.DEC_UPSTREAM)
@pytest.mark.parametrize('shape', SMALL, ids=lambda s: 'x'.join(str(v) for v in s))
@pytest.mark.parametrize('kind', RA.KINDS)
def test_loop_ref_against_torch_nn_modules(kind, shape, upstream):
    c = RA.att_case(kind, shape)
    a, b = RA.att_ref_run(c, upstream=upstream), RA.att_ref_run(c, upstream=upstream, loop=RA.att_loop_modules)
    assert set(a) == set(b) == {'zs', 'w', 'd_enc', 'd_pre'} | set(RA.DEC_KEYS) | set(RA.ATT_KEYS[kind])
    for k in sorted(a):
        assert a[k].shape == b[k].shape, k
        scale = max(a[k].abs().max().item(), 1e-30)
        assert (a[k] - b[k]).abs().max().item() <= 1e-10 * scale + 1e-13, (k, (a[k] - b[k]).abs().max().item(), scale)


def test_coverage_state_is_exercised():
    """One frame: w = 1 at every step whatever the energies; coverage with wvec = 0 is add."""
    c = RA.att_case('coverage', (5, 37, 6, 32, 24, 12, 3, 4))
    z = dict(c, Pm=dict(c['Pm'], wvec_w=torch.zeros_like(c['Pm']['wvec_w']), wvec_b=torch.zeros_like(c['Pm']['wvec_b'])))
    add = dict(c, kind='add', Pm={k: v for k, v in c['Pm'].items() if not k.startswith('wvec')})
    a, b, full = RA.att_ref_run(z), RA.att_ref_run(add), RA.att_ref_run(c)
    assert (a['w'] - b['w']).abs().max().item() < 1e-14
    assert (full['w'] - b['w']).abs().max().item() > 1e-3
    one = RA.att_ref_run(RA.att_case('coverage', (2, 1, 2, 4, 4, 4, 1, 0)))
    assert torch.equal(one['w'], torch.ones_like(one['w']))


@functools.lru_cache(maxsize=None)
def refs(kind, shape, upstream):
    c = RA.att_case(kind, shape)
    return RA.att_ref_run(c, upstream=upstream), RA.att_ref_run(c, torch.float32, upstream)


@pytest.mark.parametrize('upstream', R.DEC_UPSTREAM)
@pytest.mark.parametrize('shape', [s for s, _ in RA.ATT_SHAPES], ids=lambda s: 'x'.join(str(v) for v in s))
@pytest.mark.parametrize('kind', RA.KINDS)
def test_bars_are_meaningful_on_the_gpu_tests_inputs(kind, shape, upstream):
    f64, f32 = refs(kind, shape, upstream)
    for k in sorted(f64):
        if k == 'gvec_b':
            assert f64[k].abs().max().item() < 1e-12           # analytically zero
            continue
        if k in ('zs', 'w'):
            R.margin_ok(k, f32[k], f64[k], R.BAR_DEC_OUT)
        else:
            R.margin_ok(k, f32[k], f64[k], R.BAR_DEC_GRAD, R.ATOL_DEC_GRAD)


# ---------------------------------------------------------------------------------------------
# host side
# ---------------------------------------------------------------------------------------------
def _opt(atype, **kw):
    import __graft_entry__ as g
    return argparse.Namespace(**{**vars(g._tiny_opt()), 'atype': atype, **kw})


@pytest.mark.parametrize('kind', RA.KINDS)
def test_e2e_builds_the_type_with_the_reference_names(golden_dir, kind):
    from robust_e2e_gan_amd.model import e2e_attention as att
    from robust_e2e_gan_amd.model.e2e_model import E2E, ShareE2E
    p, _ = fixture_params(golden_dir, kind)
    cls = dict(dot=att.AttDot, add=att.AttAdd, coverage=att.AttCov, coverage_location=att.AttCovLoc)[kind]
    for model in (E2E, ShareE2E):
        m = model(_opt(kind))
        assert type(m.att) is cls and m.att.kind == kind and m.dec.att is m.att
        have = {k: tuple(v.shape) for k, v in m.state_dict().items()}
        want = {k: tuple(v.shape) for k, v in p.items()}
        want.update({'dec.' + k: s for k, s in want.items() if k.startswith('att.')})       # ``att`` is registered twice, as upstream
        assert have == want, set(have) ^ set(want)
    names = {k[4:] for k in want if k.startswith('att.')}
    assert names == {'dot': {'mlp_enc.weight', 'mlp_enc.bias', 'mlp_dec.weight', 'mlp_dec.bias'},
                     'add': {'mlp_enc.weight', 'mlp_enc.bias', 'mlp_dec.weight', 'gvec.weight', 'gvec.bias'},
                     'coverage': {'mlp_enc.weight', 'mlp_enc.bias', 'mlp_dec.weight', 'wvec.weight', 'wvec.bias', 'gvec.weight', 'gvec.bias'},
                     'coverage_location': {'mlp_enc.weight', 'mlp_enc.bias', 'mlp_dec.weight', 'mlp_att.weight', 'loc_conv.weight', 'gvec.weight',
                                           'gvec.bias'}}[kind]
    if kind == 'coverage':
        assert want['att.wvec.weight'] == (18, 1) and want['att.wvec.bias'] == (18,)


@pytest.mark.parametrize('kind', RA.KINDS)
def test_state_dict_round_trip(golden_dir, kind):
    from robust_e2e_gan_amd.model.e2e_model import E2E
    p, _ = fixture_params(golden_dir, kind)
    sd = dict(p)
    sd.update({'dec.' + k: v for k, v in p.items() if k.startswith('att.')})
    m = E2E(_opt(kind))
    m.load_state_dict(sd, strict=True)
    back = m.state_dict()
    assert set(back) == set(sd) and all(torch.equal(back[k], sd[k]) for k in sd)
    m2 = E2E(_opt(kind))
    m2.load_state_dict(back, strict=True)
    assert all(torch.equal(a, b) for a, b in zip(m.parameters(), m2.parameters()))
    # both registrations are ONE module: no parameter counted twice
    assert len(list(m.parameters())) == len({id(q) for q in m.parameters()})
    # another type's checkpoint does not load silently
    other = 'add' if kind != 'add' else 'dot'
    with pytest.raises(RuntimeError):
        E2E(_opt(other)).load_state_dict(sd, strict=True)


@pytest.mark.parametrize('atype', ['noatt', 'location2d', 'location_recurrent', 'multi_head_dot', 'multi_head_add', 'multi_head_loc',
                                   'multi_head_multi_res_loc'])
def test_e2e_still_refuses_the_other_types_and_says_which_it_has(atype):
    from robust_e2e_gan_amd.lib import Re2eError
    from robust_e2e_gan_amd.model.e2e_model import E2E
    with pytest.raises(Re2eError) as e:
        E2E(_opt(atype))
    msg = str(e.value)
    assert atype in msg and 'out of scope' in msg
    assert all(k in msg for k in ('location', 'dot', 'add', 'coverage', 'coverage_location'))


def test_non_softmax_activation_is_still_refused():
    from robust_e2e_gan_amd.model.e2e_attention import AttLoc
    with pytest.raises(NotImplementedError, match='softmax'):
        AttLoc(20, 14, 18, 4, 5, 'sigmoid')


def test_decoder_names_the_kind_for_the_loop_and_the_search(golden_dir):
    from robust_e2e_gan_amd.lib import Re2eError
    from robust_e2e_gan_amd.model import e2e_decoder as D
    assert D.att_kind({}) == 'location'                     # parameter dicts from before the other types: the step they always meant
    for kind in RA.KINDS:
        p, _ = fixture_params(golden_dir, kind)
        got = D.att_params(p, '', kind)
        assert set(got) == set(RA.ATT_KEYS[kind])
    with pytest.raises(Re2eError, match='no decoder step'):
        D.att_params({}, '', 'location2d')
