"""Encoder.encode_batch and the two encoder arms of E2E.recognize_batch, on the model and the three utterances of tests/golden/recog_tiny.npz
(37 / 29 / 20 frames of 80 features; the plans name the fused Winograd kernels for conv1_2, conv2_1 and conv2_2 at these shapes, so the
valid-height stack runs and nothing falls back -- asserted).

The VGG part of a padded batch is held to the per-utterance one BIT FOR BIT; the encoder states are held to oracle.nets.encoder_forward in
float64 on the CPU, utterance by utterance, at 8 x the distance of the same oracle in float32 from float64 (of max |h|) -- the batched path
and the per-utterance path against the SAME bar, which therefore never comes from the code under test.

Measured on an MI355X when the module was written: see the docstring of test_encode_batch_states_against_float64."""
import numpy as np
import pytest
import torch

from test_modules_gpu import DEV
from test_recog_batch_gpu import CHARS, _args, _same, _tiny

pytestmark = pytest.mark.gpu


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _vgg_of_batch(enc, xs, lens):
    """encode_batch with a recorder on VGG2L.pack_tm -> (hpad, hlens, the VGG output (T', U, 128 F') as the recurrent stack received it, its lengths)."""
    seen = []
    orig = enc.enc1.pack_tm

    def spy(hs, ilens_per_branch):
        out = orig(hs, ilens_per_branch)
        seen.append((out[0].clone(), list(out[1]), [list(l) for l in ilens_per_branch]))
        return out

    enc.enc1.pack_tm = spy
    try:
        hpad, hlens = enc.encode_batch(xs, lens)
    finally:
        del enc.enc1.pack_tm
    return hpad, hlens, seen


def _setup(golden_dir):
    base, asr, feats, lens = _tiny(golden_dir)
    assert lens == [37, 29, 20] and feats.shape == (3, 37, 80)
    asr.eval()
    assert asr.enc.enc1.valid_stack_ok(3, 37, 80), 'the plans no longer name the Winograd kernels for the tiny VGG stack: this module would test the fallback'
    return base, asr, feats, lens


def test_encode_batch_vgg_part_is_the_single_utterance_one_bit_for_bit(golden_dir):
    """The padded batch, the same batch with NaN in its padding rows (the caller's tensor comes back untouched) and the batch in the order
    (2, 0, 1): the VGG output below each pooled length is, bit for bit, VGG2L.forward_tm of the utterance alone; so are the encoder states of
    the NaN-padded run those of the zero-padded one."""
    base, asr, feats, lens = _setup(golden_dir)
    enc = asr.enc
    with torch.no_grad():
        alone = [enc.enc1.forward_tm(feats[u:u + 1, :T].to(DEV), [T]) for u, T in enumerate(lens)]
        pl = enc.enc1.pooled_lens(lens)
        assert [a[1] for a in alone] == [[p] for p in pl] and pl == [10, 8, 5]
        nanpad = feats.clone()
        for u, T in enumerate(lens):
            nanpad[u, T:] = float('nan')
        nan_dev = nanpad.to(DEV)
        perm = [2, 0, 1]
        runs = {}
        for name, xs, ls, order in (('zeros', feats.to(DEV), lens, [0, 1, 2]), ('nan', nan_dev, lens, [0, 1, 2]),
                                    ('perm', feats[perm].to(DEV), [lens[u] for u in perm], perm)):
            hpad, hlens, seen = _vgg_of_batch(enc, xs, ls)
            assert len(seen) == 1 and seen[0][2] == [ls], '%s: the batch was not encoded as one group through the valid-height stack' % name
            h_tm, nl, _ = seen[0]
            assert nl == [pl[u] for u in order] and hlens == nl and tuple(hpad.shape[:2]) == (3, 10)
            for j, u in enumerate(order):
                a = alone[u][0][:pl[u], 0]
                assert torch.isfinite(a).all()
                assert torch.equal(h_tm[:pl[u], j], a), '%s: VGG output of utterance %d differs from the utterance alone (max %.3e)' % (
                    name, u, (h_tm[:pl[u], j] - a).abs().max().item())
                assert bool((h_tm[pl[u]:, j] == 0).all()), '%s: the re-pad beyond the pooled length is not zero' % name
            runs[name] = (hpad, hlens)
        assert torch.equal(_bits(nan_dev), _bits(nanpad.to(DEV))), "encode_batch wrote into the caller's tensor"
        for u in range(3):
            assert torch.equal(runs['nan'][0][u, :pl[u]], runs['zeros'][0][u, :pl[u]]), 'NaN in the padding rows reached the states of utterance %d' % u
            assert torch.isfinite(runs['zeros'][0][u, :pl[u]]).all()


def test_encode_batch_states_against_float64(golden_dir):
    """Encoder states of the batch (in order and in the order (2, 0, 1)) and of the per-utterance path against oracle.nets.encoder_forward in
    float64, per utterance, as a fraction of max |h|; bar = 8 x the worst distance of the same oracle in float32.

    Measured on an MI355X when the module was written (worst of the three utterances): fp32 oracle 8.91e-7 -> bar 7.13e-6; batched 8.63e-7,
    batched (2, 0, 1) 8.63e-7, per utterance 8.63e-7."""
    from oracle import nets
    base, asr, feats, lens = _setup(golden_dir)
    p32 = {k[2:]: torch.from_numpy(v) for k, v in base.items() if k.startswith('p.enc.')}
    p64 = {k: v.double() for k, v in p32.items()}
    h64, d32 = [], 0.0
    with torch.no_grad():
        for u, T in enumerate(lens):
            a, nl = nets.encoder_forward(p64, feats[u:u + 1, :T].double(), [T], 2)
            b, _ = nets.encoder_forward(p32, feats[u:u + 1, :T], [T], 2)
            h64.append(a[0, :nl[0]])
            d32 = max(d32, (b[0, :nl[0]].double() - h64[-1]).abs().max().item() / h64[-1].abs().max().item())
        bar = 8 * d32
        dist = lambda h, u: (h.double().cpu() - h64[u]).abs().max().item() / h64[u].abs().max().item()
        perm = [2, 0, 1]
        hb, lb = asr.enc.encode_batch(feats.to(DEV), lens)
        hp, lp = asr.enc.encode_batch(feats[perm].to(DEV), [lens[u] for u in perm])
        each = [asr.enc(feats[u:u + 1, :T].to(DEV), [T]) for u, T in enumerate(lens)]
        got = {'batched': max(dist(hb[u, :lb[u]], u) for u in range(3)),
               'batched (2, 0, 1)': max(dist(hp[j, :lp[j]], u) for j, u in enumerate(perm)),
               'per utterance': max(dist(each[u][0][0, :each[u][1][0]], u) for u in range(3))}
    assert lb == [10, 8, 5] and lp == [5, 10, 8]
    print('ERR encoder states: fp32 oracle %.2e -> bar %.2e; %s' % (d32, bar, '; '.join('%s %.2e' % kv for kv in got.items())))
    for name, d in got.items():
        assert d <= bar, '%s: %.3e of max |h| from float64, bar %.3e (8 x the fp32 oracle: %.3e)' % (name, d, bar, d32)


def test_recognize_batch_encoder_arms_agree(golden_dir):
    """encode='batch' and encode='each' return the same label sequences for the four search configurations, scores within 1e-5 max(1, |score|)
    (the batched products see other row counts and may run on another plan), both the reference's n-best lists; the search is handed
    exactly each utterance's own frames -- no padding row of ``hpad``."""
    from test_oracle_golden import RECOG_CONFIGS, check_nbest
    base, asr, feats, lens = _setup(golden_dir)
    handed = []
    orig = asr.dec.recognize_beam_batch

    def spy(hs, lpzs, *a, **k):
        handed.append(([int(h.shape[0]) for h in hs], None if lpzs is None else [int(l.shape[0]) for l in lpzs]))
        return orig(hs, lpzs, *a, **k)

    asr.dec.recognize_beam_batch = spy
    try:
        for name, beam, penalty, ctcw, maxr, minr, nbest in RECOG_CONFIGS:
            args = _args(beam, penalty, ctcw, maxr, minr, nbest)
            arms = {k: asr.recognize_batch(feats, lens, args, CHARS, encode=k) for k in ('batch', 'each')}
            for u in range(3):
                _same(arms['batch'][u], arms['each'][u], 1e-5)
                for k in arms:
                    check_nbest(arms[k][u], base, name, u)
            for hl, ll in handed[-2:]:
                assert hl == [10, 8, 5] and ll == (hl if ctcw > 0.0 else None), (name, hl, ll)
    finally:
        del asr.dec.recognize_beam_batch
    assert len(handed) == 8
    with pytest.raises(Exception):
        asr.recognize_batch(feats, lens, _args(3, 0.0, 0.0, 0.0, 0.0, 3), CHARS, encode='other')


def test_encode_batch_guards(golden_dir):
    """Gradients enabled on a model with trainable parameters: refused.  A batch of equal lengths (no padding): the VGG part equals the plain
    VGG2L.forward_tm of the batch bit for bit."""
    from robust_e2e_gan_amd.lib import Re2eError
    base, asr, feats, lens = _setup(golden_dir)
    x = feats[:, :20].contiguous().to(DEV)
    with pytest.raises(Re2eError):
        asr.enc.encode_batch(x, [20, 20, 20])
    with torch.no_grad():
        plain, nl = asr.enc.enc1.forward_tm(x, [20, 20, 20])
        hpad, hlens, seen = _vgg_of_batch(asr.enc, x, [20, 20, 20])
        ref, rl = asr.enc(x, [20, 20, 20])
    assert len(seen) == 1 and nl == [5, 5, 5] == hlens == rl
    assert torch.equal(seen[0][0], plain), 'equal lengths: the valid-height stack differs from the plain one'
    assert torch.equal(hpad, ref)
    assert np.isfinite(hpad.cpu().numpy()).all()


def _held_to_float64(tag, runs, ref):
    """``runs``: name -> list of per-utterance states; ``ref(u, dtype)`` the CPU oracle of utterance u.  Bar: 8 x the worst distance of the
    float32 oracle from the float64 one, of max |h|; every run is held to it."""
    h64 = [ref(u, torch.float64) for u in range(len(next(iter(runs.values()))))]
    d32 = max((ref(u, torch.float32).double() - h).abs().max().item() / h.abs().max().item() for u, h in enumerate(h64))
    got = {}
    for name, hs in runs.items():
        assert [tuple(h.shape) for h in hs] == [tuple(h.shape) for h in h64], name
        assert all(bool(torch.isfinite(h).all()) for h in hs), name
        got[name] = max((h.double().cpu() - r).abs().max().item() / r.abs().max().item() for h, r in zip(hs, h64))
    print('ERR %s: fp32 oracle %.2e -> bar %.2e; %s' % (tag, d32, 8 * d32, '; '.join('%s %.2e' % kv for kv in got.items())))
    for name, d in got.items():
        assert d <= 8 * d32, '%s %s: %.3e of max |h| from float64, bar %.3e' % (tag, name, d, 8 * d32)


def test_encode_batch_in_several_groups(golden_dir):
    """Five utterances (the three of the fixture as 1, 0, 2, 0, 1: 29 / 37 / 20 / 37 / 29 frames, NaN in the padding) with ``group=2``: three
    groups cut from the length-sorted utterances -- (37, 37), (29, 29), (20) frames, each padded to ITS longest, T' = 10 / 8 / 5 -- whose
    results go back to the caller's positions.  The VGG output of every group is bit for bit the single utterances'; the states are held to
    the float64 oracle per utterance like those of the one-group call, and equal it where a group is the same launch on the same rows
    (duplicates inside a group).

    Measured on an MI355X when the test was written: fp32 oracle 8.91e-7 -> bar 7.13e-6; groups of 2 8.63e-7, one group 7.38e-7."""
    from oracle import nets
    base, asr, feats, lens = _setup(golden_dir)
    pick = [1, 0, 2, 0, 1]
    ls = [lens[u] for u in pick]
    xs = feats[pick].clone()
    for j, T in enumerate(ls):
        xs[j, T:] = float('nan')
    p32 = {k[2:]: torch.from_numpy(v) for k, v in base.items() if k.startswith('p.enc.')}

    def ref(j, dtype):
        p = {k: v.to(dtype) for k, v in p32.items()}
        with torch.no_grad():
            h, nl = nets.encoder_forward(p, xs[j:j + 1, :ls[j]].to(dtype), [ls[j]], 2)
        return h[0, :nl[0]]

    seen = []
    orig = asr.enc.enc1.pack_tm

    def spy(hs, ilens_per_branch):
        out = orig(hs, ilens_per_branch)
        seen.append(([list(l) for l in ilens_per_branch], out[0].clone()))
        return out

    with torch.no_grad():
        alone = {u: asr.enc.enc1.forward_tm(feats[u:u + 1, :lens[u]].to(DEV), [lens[u]])[0][:, 0] for u in range(3)}
        asr.enc.enc1.pack_tm = spy
        try:
            hg, lg = asr.enc.encode_batch(xs.to(DEV), ls, group=2)
        finally:
            del asr.enc.enc1.pack_tm
        h1, l1 = asr.enc.encode_batch(xs.to(DEV), ls)
    assert [s[0] for s in seen] == [[[37, 37]], [[29, 29]], [[20]]], [s[0] for s in seen]
    for (gl, h_tm), u in zip(seen, (0, 1, 2)):
        for j in range(len(gl[0])):
            assert torch.equal(h_tm[:, j], alone[u]), 'group of %r frames: VGG output differs from the utterance alone' % gl
    pl = [8, 10, 5, 10, 8]
    assert lg == pl == l1 and tuple(hg.shape[:2]) == (5, 10) == tuple(h1.shape[:2])
    assert torch.equal(hg[1, :10], hg[3, :10]) and torch.equal(hg[0, :8], hg[4, :8]), 'duplicates inside one group differ'
    _held_to_float64('vggblstmp in groups of 2', {'groups of 2': [hg[j, :pl[j]] for j in range(5)], 'one group': [h1[j, :pl[j]] for j in range(5)]}, ref)


@pytest.mark.parametrize('etype', ['blstmp', 'blstm'])
def test_encode_batch_recurrent_only_encoders(etype):
    """blstm / blstmp (no VGG front end): four utterances of 23 / 9 / 17 / 3 frames of 16 features in that order, NaN in the padding, as one
    group and with ``group=3`` (sorted: (23, 17, 9), (3)), against oracle.nets in float64 per utterance; the per-utterance encoder is held to
    the same bar.

    Measured on an MI355X when the test was written: blstmp fp32 oracle 2.06e-7 -> bar 1.64e-6, all three paths 2.16e-7; blstm 2.64e-7 ->
    2.11e-6, all three paths 2.64e-7."""
    from oracle import nets
    from robust_e2e_gan_amd.model.e2e_encoder import Encoder
    torch.manual_seed(31)
    idim, elayers, eunits, eprojs = 16, 2, 24, 20
    enc = Encoder(etype, idim, elayers, eunits, eprojs, [1] * (elayers + 1), 'skip', 0.0)
    for p_ in enc.parameters():
        p_.data.uniform_(-0.3, 0.3)
    p32 = {'enc.' + k: v.detach().clone() for k, v in enc.state_dict().items()}
    enc = enc.to(DEV).eval()
    ls = [23, 9, 17, 3]
    xs = torch.randn(4, 23, idim, generator=torch.Generator().manual_seed(32))
    for j, T in enumerate(ls):
        xs[j, T:] = float('nan')

    def ref(j, dtype):
        p = {k: v.to(dtype) for k, v in p32.items()}
        x = xs[j:j + 1, :ls[j]].to(dtype)
        with torch.no_grad():
            if etype == 'blstmp':
                return nets.blstmp_forward(p, x, [ls[j]], elayers, pre='enc.enc1.')[0][0]
            w = {k[len('enc.enc1.nblstm.'):]: v for k, v in p.items() if k.startswith('enc.enc1.nblstm.')}
            y = x
            for l in range(elayers):
                y = nets._bilstm(y, [ls[j]], w, '', l)
            return torch.tanh(torch.nn.functional.linear(y[0], p['enc.enc1.l_last.weight'], p['enc.enc1.l_last.bias']))

    with torch.no_grad():
        h1, l1 = enc.encode_batch(xs.to(DEV), ls)
        hg, lg = enc.encode_batch(xs.to(DEV), ls, group=3)
        each = [enc(xs[j:j + 1, :T].to(DEV), [T])[0][0, :T] for j, T in enumerate(ls)]
    assert l1 == ls == lg and tuple(h1.shape) == (4, 23, eprojs) == tuple(hg.shape)
    _held_to_float64(etype, {'one group': [h1[j, :T] for j, T in enumerate(ls)], 'groups of 3': [hg[j, :T] for j, T in enumerate(ls)],
                             'per utterance': each}, ref)
